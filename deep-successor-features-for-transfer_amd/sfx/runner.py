"""Host-side env-step loop of SF-DQN driving the libsfx engine.

Mirrors Agent.next_sample (agents/agent.py:195-261) + SFDQN.train_agent for the two
schedules the reference has:

  * "all":    agents/sfdqn.py:47-60 over features/deep.py (main_sfdqn_torch.py):
              LMS reward fit on the active task, every head updated per env step, GPI next
              actions, loss = l1.
  * "active": sfdqn.py:462-471 / agents/sfdqn_sequential.py:63-76: only the active head is
              updated (with l2 + Adam-trained w), next actions by GPI or own ψ (use_gpi).
  * "tsf":    tsfdqn.py:566-580 / tsfdqn_nf.py:598-612: only the active head is updated, by
              TSFDQN.update_successor (φ̃ from g_i and the shared h; the engine must have
              been set up with SFEngine.tsf_setup).

The environment is a synthetic Reacher-shape task: s ~ N(0,1)^n_s,
φ ~ U[0,1)^d, r = φ·w_true with one-hot w_true (tasks/reacher.py:85-88), γ constant,
episodes of T_ep steps.  Replay is a host ring (agents/buffer.py:34-82) sampled uniformly;
each step's device inputs (the minibatch, the new transition's φ/r, the next state) travel
in ONE pinned host->device copy.
"""
from __future__ import annotations

import numpy as np
import torch

from .engine import SFEngine


class SynthReacher:
    """Synthetic Reacher-shape task (never terminates, like tasks/reacher.py:112)."""

    def __init__(self, n_s: int, A: int, d: int, task_index: int, rng: np.random.Generator):
        self.n_s, self.A, self.d, self.task_index, self.rng = n_s, A, d, task_index, rng
        self.w_true = np.zeros(d, dtype=np.float32)
        self.w_true[task_index % d] = 1.0

    def initialize(self) -> np.ndarray:
        return self.rng.standard_normal(self.n_s, dtype=np.float32)

    def transition(self, a: int):
        s1 = self.rng.standard_normal(self.n_s, dtype=np.float32)
        phi = self.rng.random(self.d, dtype=np.float32)
        r = float(phi @ self.w_true)
        return s1, phi, r, False


class SynthHopper(SynthReacher):
    """Synthetic Hopper-shape task (BASELINE config C3: |s|=11, 27 actions, d=50): like
    SynthReacher, but an episode ends with probability `p_end` per step (γ = 0 then), the
    way tasks/hopper_phi.py's falls do."""

    def __init__(self, n_s: int, A: int, d: int, task_index: int, rng: np.random.Generator, p_end: float = 0.01):
        super().__init__(n_s, A, d, task_index, rng)
        self.p_end = p_end

    def transition(self, a: int):
        s1, phi, r, _ = super().transition(a)
        return s1, phi, r, bool(self.rng.random() < self.p_end)


def draw_test_schedule(E: int, horizon: int, epsilon: float, n_actions: int) -> np.ndarray:
    """The exploration schedule of E sequential test episodes of ``horizon`` steps, drawn from Python's ``random``
    in the reference's order (SFDQN.get_test_action, agents/sfdqn.py:127-128: per step one ``random.random()``
    and, when it is <= epsilon, one ``random.randrange(n_actions)``; task 0's steps, then task 1's, ...).  Entry
    [e, j] is the explored action or -1 for a greedy step.  For ``NativeEnvLoop.test_phase(explore=...)``, so a
    run keeps the reference's own random stream; the draws are ``sfx.lockstep``'s (one shared function)."""
    from .lockstep import _draw_schedule

    return np.asarray(_draw_schedule(int(E), int(horizon), float(epsilon), int(n_actions)),
                      dtype=np.int32).reshape(int(E), int(horizon))


def draw_tsf_test_schedule(E: int, horizon: int, epsilon: float, n_actions: int, diag: bool = False) -> np.ndarray:
    """The exploration schedule of E sequential TSF test episodes of ``horizon`` steps, drawn from Python's
    ``random`` in the reference's order (agents/tsfdqn_sequential.py:377-381 over :399-402: per step the draws of
    ``get_test_action`` at s and then at s1, each one ``random.random()`` and, when it is <= epsilon, one
    ``random.randrange(n_actions)``; task 0's steps, then task 1's, ...).  Entry [e, j] = (explored a, explored
    a1), -1 for a greedy choice.  diag: also consume the binding's per-step diagnostic draw (:502), as
    ``sfx.lockstep`` does for an agent that prints.  For ``NativeEnvLoop.tsf_test_phase(explore=...)``; the
    draws are ``sfx.lockstep``'s (one shared function)."""
    from . import lockstep

    sched = lockstep._tsf_draw_schedule(int(E), int(horizon), float(epsilon), int(n_actions), bool(diag))
    return np.asarray([[(xa, xa1) for xa, xa1, _ in row] for row in sched],
                      dtype=np.int32).reshape(int(E), int(horizon), 2)


TSF_TEST_HP = ("gamma", "beta", "lasso", "lr_w", "wd_w", "lr_omega", "wd_omega", "lr_omega_decay")


def test_phase_steps(n_samples: int, n_test_ev: int) -> list:
    """The training steps t of one task's ``n_samples`` after which SFDQN.train evaluates
    (agents/sfdqn.py:105-111: ``if t % n_test_ev == 0``)."""
    return list(range(0, int(n_samples), int(n_test_ev)))


test_phase_steps.__test__ = False  # a helper, not a pytest case


# ---- what NativeEnvLoop's three test-phase wrappers share ----

def _is_f32_on(t, device, dim=None) -> bool:
    """t is a contiguous float32 tensor on ``device`` (of ``dim`` dimensions when given)."""
    return (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and (dim is None or t.dim() == dim)
            and t.is_contiguous() and t.device == torch.device(device))


def _explore_array(explore, shape):
    """The caller's exploration schedule as a contiguous int32 array of ``shape``, or None."""
    if explore is None:
        return None
    ex = np.ascontiguousarray(np.asarray(explore, dtype=np.int32))
    if ex.shape != shape:
        raise ValueError(f"explore: an int array [{', '.join(str(n) for n in shape)}]")
    return ex


def _lockstep_call(C, check, fn, what, head, explore, E, horizon, want_actions, comps=(), draws=()):
    """``fn(*head, explore, returns, loss sums, steps, actions)`` with fresh outputs (at least one row and one step,
    so that a refused E = 0 or horizon = 0 still hands over valid pointers), sliced to E rows and horizon steps."""
    n = max(E, 1)
    ret, loss, steps = np.zeros(n, np.float64), np.zeros((n,) + comps, np.float64), np.zeros(n, np.int64)
    acts = np.full((n, max(horizon, 1)) + draws, -1, np.int64) if want_actions else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    check(fn(*head, ptr(explore), ptr(ret), ptr(loss), ptr(steps), ptr(acts)), what)
    out = (ret[:E], loss[:E], steps[:E])
    return out + (acts[:E, :horizon],) if want_actions else out


class Staging:
    """One pinned host buffer + one device buffer with typed views at fixed offsets."""

    def __init__(self, fields, device):
        self.offsets, off = {}, 0
        for name, shape, dtype in fields:
            n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            self.offsets[name] = (off, shape, dtype)
            off += (n + 15) // 16 * 16
        self.nbytes = off
        self.host = torch.empty(off, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(off, dtype=torch.uint8, device=device)
        self.h = {k: self._view(self.host, k).numpy() for k in self.offsets}
        self.d = {k: self._view(self.dev, k) for k in self.offsets}

    def _view(self, buf, name):
        off, shape, dtype = self.offsets[name]
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return buf[off:off + n].view(dtype).view(*shape)

    def upload(self):
        self.dev.copy_(self.host, non_blocking=True)


class Replay:
    """Uniform replay ring (agents/buffer.py:34-82) with arrays instead of object tuples."""

    def __init__(self, capacity: int, n_s: int, d: int, rng: np.random.Generator):
        self.cap, self.rng = capacity, rng
        self.s = np.zeros((capacity, n_s), np.float32)
        self.s1 = np.zeros((capacity, n_s), np.float32)
        self.phi = np.zeros((capacity, d), np.float32)
        self.r = np.zeros(capacity, np.float32)
        self.a = np.zeros(capacity, np.int64)
        self.gamma = np.zeros(capacity, np.float32)
        self.index = 0
        self.size = 0

    def append(self, s, a, r, phi, s1, gamma):
        i = self.index
        self.s[i], self.a[i], self.r[i], self.phi[i], self.s1[i], self.gamma[i] = s, a, r, phi, s1, gamma
        self.size = min(self.size + 1, self.cap)
        self.index = (i + 1) % self.cap

    def sample_into(self, st: Staging, B: int) -> bool:
        if self.size < B:
            return False
        idx = self.rng.integers(0, self.size, B)
        np.take(self.s, idx, axis=0, out=st.h["s"])
        np.take(self.s1, idx, axis=0, out=st.h["s1"])
        np.take(self.phi, idx, axis=0, out=st.h["phi"])
        if "r" in st.h:
            np.take(self.r, idx, out=st.h["r"].reshape(-1))
        np.take(self.a, idx, out=st.h["a"])
        np.take(self.gamma, idx, out=st.h["gamma"])
        return True


class EnvLoop:
    """The training env-step loop of one active task over an SFEngine of T heads."""

    def __init__(self, engine: SFEngine, schedule: str = "all", batch: int = 32, capacity: int = 1_000_000,
                 gamma: float = 0.9, epsilon: float = 0.1, alpha_w: float = 1e-3, episode_len: int = 500,
                 use_gpi: bool = True, seed: int = 1, task_cls=SynthReacher):
        assert schedule in ("all", "active", "tsf")
        self.eng, self.schedule, self.B = engine, schedule, batch
        self.gamma, self.epsilon, self.alpha_w, self.T_ep, self.use_gpi = gamma, epsilon, alpha_w, episode_len, use_gpi
        e = engine
        self.rng = np.random.default_rng(seed)
        self.tasks = [task_cls(e.n_s, e.A, e.d, t, self.rng) for t in range(e.T)]
        self.replay = Replay(capacity, e.n_s, e.d, self.rng)
        self.st = Staging([("s", (batch, e.n_s), torch.float32), ("s1", (batch, e.n_s), torch.float32),
                           ("phi", (batch, e.d), torch.float32), ("r", (batch,), torch.float32),
                           ("a", (batch,), torch.int64), ("gamma", (batch,), torch.float32),
                           ("snext", (1, e.n_s), torch.float32), ("phi1", (e.d,), torch.float32),
                           ("r1", (1,), torch.float32)], e.device)
        self.losses = torch.zeros(max(e.T, 1), 3, device=e.device)
        self.sel_host = torch.zeros(2, dtype=torch.long, pin_memory=True)
        self.gpi_counters = np.zeros((e.T, e.T), dtype=np.int64)
        self.set_task(0)

    def set_task(self, index: int):
        """Agent.set_active_training_task (agents/agent.py:121-139)."""
        self.task_index = index
        self.task = self.tasks[index]
        self.steps_in_episode = 0
        self.s = self.task.initialize()
        self.st.h["snext"][0] = self.s
        self.st.upload()
        if self.schedule == "all":
            self.eng.step_all(s_next=self.st.d["snext"], task_index=index, sel_use_gpi=self.use_gpi)
            c, a, _ = self.eng.step_finish()
            self.sel = (c, a)
        else:
            self._issue_select()

    def prefill(self, n: int):
        """Random transitions into the replay (warm-up only; not an env step)."""
        for _ in range(n):
            s = self.task.initialize()
            a = int(self.rng.integers(self.eng.A))
            s1, phi, r, _ = self.task.transition(a)
            self.replay.append(s, a, r, phi, s1, self.gamma)

    def _issue_select(self):
        e = self.eng
        sel = e.select_action(self.st.d["snext"], self.task_index, self.use_gpi)
        self.sel_host.copy_(sel, non_blocking=True)
        self.sel_event = torch.cuda.Event()
        self.sel_event.record()

    def _greedy(self):
        if self.schedule == "all":
            return self.sel
        self.sel_event.synchronize()
        return int(self.sel_host[0]), int(self.sel_host[1])

    def step(self):
        """One env step: GPI action (computed by the previous step), ε-greedy, transition, train."""
        c, a_greedy = self._greedy()
        self.gpi_counters[self.task_index, c] += 1
        if self.rng.random() <= self.epsilon:
            a = int(self.rng.integers(self.eng.A))
        else:
            a = a_greedy
        s1, phi, r, terminal = self.task.transition(a)
        g = 0.0 if terminal else self.gamma
        st = self.st
        self.replay.append(self.s, a, r, phi, s1, g)
        have = self.replay.sample_into(st, self.B)
        self.steps_in_episode += 1
        s_next = s1
        if terminal or self.steps_in_episode >= self.T_ep:  # new episode (agent.py:211-220, 248-249)
            s_next = self.task.initialize()
            self.steps_in_episode = 0
        st.h["phi1"][:] = phi
        st.h["r1"][0] = r
        st.h["snext"][0] = s_next
        st.upload()
        d, e = st.d, self.eng
        if self.schedule == "all":
            if have:
                e.step_all(d["s"], d["a"], d["phi"], d["s1"], d["gamma"], use_gpi=True, lms_task=self.task_index,
                           lms_phi=d["phi1"], lms_r=d["r1"], lms_alpha=self.alpha_w, s_next=d["snext"],
                           task_index=self.task_index, sel_use_gpi=self.use_gpi, losses=self.losses)
            else:
                e.step_all(lms_task=self.task_index, lms_phi=d["phi1"], lms_r=d["r1"], lms_alpha=self.alpha_w,
                           s_next=d["snext"], task_index=self.task_index, sel_use_gpi=self.use_gpi)
            c, a, _ = e.step_finish()
            self.sel = (c, a)
        else:
            upd = e.tsf_update if self.schedule == "tsf" else e.update
            if have:
                upd(self.task_index, d["s"], d["a"], d["r"], d["phi"], d["s1"], d["gamma"], self.use_gpi,
                    losses=self.losses[0])
            self._issue_select()
        self.s = s_next

    def run(self, n: int):
        for _ in range(n):
            self.step()


class NativeEnvLoop:
    """The env-step loop of EnvLoop run by libsfx's native runner (include/sfx.h, sfx_runner_*):
    C++ env + replay ring on the host, one pre-launched hipGraph per env step whose gate kernel
    waits for the host's inputs.  schedule: "all" (main_sfdqn_torch.py), "active" (sfdqn.py /
    agents/sfdqn_sequential.py: the active head with l2 and an Adam-trained w, no LMS), "tsf"
    (TSFDQN.update_successor; needs SFEngine.tsf_setup), "sharded" (the all-task step with the
    heads split over ranks, BASELINE config C4) or "sharded_tsf" (the TSF step with the heads split
    over ranks, config C5: tsf_setup + shard_setup + a communicator; the active task is a global
    index and its owner updates), "phi" (agents/sfdqn_phi.py over features/deep_phi.py: the learned-φ SF
    agent's training step -- biased GPI selection, DeepSF_PHI.update_successor of the active head; needs
    SFEngine.phi_setup / phi_setup_dims) or "tsf_phi" (agents/tsfdqn_phi.py over features/deep_tsf_phi.py;
    needs a φ setup and tsf_setup(G = d, K = 0)).  The two learned-φ schedules take phi_bias / phi_lambda:
    float32 device tensors of T elements, the tasks' reward-model biases and loss coefficients, read and
    updated in place by the steps (kept alive by the loop); phi_losses() returns what the agents log.  They
    run with the host replay only and do not look ahead.  p_end: per-step episode-end
    probability of the built-in synthetic task (0: never terminates, like tasks/reacher.py).

    env: None for the built-in synthetic Reacher-shape task, or an object with
    ``reset(task) -> s0`` and ``step(task, a) -> (s1, phi, r, terminal)`` (numpy / floats),
    called through C callbacks (agents/agent.py's Task interface: tasks/task.py).  Under the learned-φ
    schedules, and while a featurizer is set, the env's φ is not used and ``step`` may return None for it.

    featurizer: a sfx.pretrain.PreEngine, a LearntPhi or None ("active" and "tsf" only, host replay only): the
    frozen pre-trained φ net of the single-file learned-φ agents' main phase (sfdqn_phi.py:482-485, :503).  Every
    step with an update then computes its minibatch's φ rows from (s, a, s1) on the device, bit for bit what the
    net gives one row at a time; the env's and the replay's φ are never read.  "active" keeps its look-ahead,
    "tsf" does not look ahead meanwhile.  The loop keeps the engine alive; its parameters may change between
    runs, not during one.

    The SF agent's test phase (agents/sfdqn.py:105-120) runs in the runner too, under "all" and "active":
    ``set_test_env`` / ``test_phase`` step the test tasks of ``test_agent`` in lockstep between runs without
    touching training, and ``train`` is SFDQN.train's loop over both.  Under "tsf" the TSF agent's test phase
    (agents/tsfdqn_sequential.py:392-433) does: ``tsf_test_phase`` steps the test tasks in lockstep, each with its
    own (w, ω), Adam moments and ω-lr schedule, and ``train`` evaluates with it.  Under "phi" the learned-φ SF
    agent's (agents/sfdqn_phi.py:234-261) does: ``phi_test_phase`` steps the test tasks in lockstep, each with its
    own biased reward model (W row, Wb entry), and ``train`` evaluates with it (``Wb=...`` among the keywords).
    """

    FIELDS =("s", "s1", "phi", "a", "gamma", "snext", "phi1", "r1", "rb")
    SCHEDULES = {"all": 0, "active": 1, "tsf": 2, "sharded": 3, "sharded_tsf": 4, "phi": 5, "tsf_phi": 6}
    PHI_SCHEDULES = ("phi", "tsf_phi")

    def __init__(self, engine: SFEngine, batch: int = 32, capacity: int = 1_000_000, gamma: float = 0.9,
                 epsilon: float = 0.1, alpha_w: float = 1e-3, episode_len: int = 500, use_gpi: bool = True,
                 seed: int = 1, env=None, schedule: str = "all", upd_use_gpi: bool = True, p_end: float = 0.0,
                 device_replay: bool = False, phi_bias=None, phi_lambda=None, featurizer=None):
        import ctypes as C

        from ._lib import ENV_RESET_FN, ENV_STEP_FN, check, lib

        self.eng, self.B, self._lib, self._check, self._C = engine, batch, lib, check, C
        self._cbs = None
        self._test_cbs = None
        self._featurizer = None
        self.episode_len = episode_len
        reset_fn = step_fn = None
        if env is not None:
            n_s, d = engine.n_s, engine.d

            def _reset(_ctx, task, s0):
                try:
                    v = np.asarray(env.reset(task), dtype=np.float32).reshape(n_s)
                    np.ctypeslib.as_array(s0, shape=(n_s,))[:] = v
                    return 0
                except Exception:  # reported as a failed step by libsfx
                    return 1

            def _step(_ctx, task, a, s1, phi, r, term):
                try:
                    ns, ph, rr, tt = env.step(task, a)
                    np.ctypeslib.as_array(s1, shape=(n_s,))[:] = np.asarray(ns, np.float32).reshape(n_s)
                    if ph is None and (self.schedule in self.PHI_SCHEDULES or self._featurizer is not None):
                        np.ctypeslib.as_array(phi, shape=(d,))[:] = 0.0
                    else:
                        np.ctypeslib.as_array(phi, shape=(d,))[:] = np.asarray(ph, np.float32).reshape(d)
                    r[0] = float(rr)
                    term[0] = 1 if tt else 0
                    return 0
                except Exception:
                    return 1

            self._cbs = (ENV_RESET_FN(_reset), ENV_STEP_FN(_step))
            reset_fn, step_fn = self._cbs
        r = C.c_void_p()
        check(lib.sfx_runner_create(C.byref(r), engine._h, batch, capacity, gamma, epsilon, alpha_w, episode_len,
                                    1 if use_gpi else 0, seed, C.cast(reset_fn, C.c_void_p) if reset_fn else None,
                                    C.cast(step_fn, C.c_void_p) if step_fn else None, None), "sfx_runner_create")
        self._r = r
        off = (C.c_int64 * 10)()
        check(lib.sfx_runner_layout(r, off), "sfx_runner_layout")
        self.layout = {k: int(off[i]) for i, k in enumerate(self.FIELDS)}
        self.record_bytes = int(off[9])
        self.schedule = schedule
        self._phi_scalars = None
        if phi_bias is not None or phi_lambda is not None:
            self.set_phi_scalars(phi_bias, phi_lambda)
        self.set_schedule(schedule, upd_use_gpi, p_end)
        self.task_index = 0
        if featurizer is not None:
            self.set_featurizer(featurizer)
        if device_replay:
            self.set_device_replay(True)

    def set_featurizer(self, featurizer):
        """sfx_runner_featurizer: a PreEngine, a LearntPhi or None (clears it); between runs."""
        eng = getattr(featurizer, "engine", featurizer)
        if eng is not None and getattr(eng, "handle", None) is None:
            raise ValueError("featurizer: a sfx.pretrain.PreEngine, a LearntPhi over one, or None")
        self._check(self._lib.sfx_runner_featurizer(self._r, eng.handle if eng is not None else None),
                    "sfx_runner_featurizer")
        self._featurizer = eng

    def set_device_replay(self, on: bool):
        """SURVEY §8f rank 2 (opt-in; the north_star keeps the replay on the host): the ring in
        HBM, appended and sampled by each step's gate kernel; the host ring stays as a mirror."""
        self._check(self._lib.sfx_runner_device_replay(self._r, 1 if on else 0), "sfx_runner_device_replay")

    def set_schedule(self, schedule: str, upd_use_gpi: bool = True, p_end: float = 0.0):
        """sfx_runner_config: the training schedule of the next steps (between runs, before set_task)."""
        self._check(self._lib.sfx_runner_config(self._r, self.SCHEDULES[schedule], 1 if upd_use_gpi else 0,
                                                float(p_end)), "sfx_runner_config")
        self.schedule = schedule

    def set_phi_scalars(self, phi_bias, phi_lambda):
        """The learned-φ schedules' per-task reward-model biases and loss coefficients (sfx_runner_phi_scalars):
        contiguous float32 tensors of T elements on the engine's device, updated in place by the steps."""
        e = self.eng
        for name, t in (("phi_bias", phi_bias), ("phi_lambda", phi_lambda)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == e.T
                    and t.device == torch.device(e.device)):
                raise ValueError(f"{name}: a contiguous float32 tensor of T = {e.T} elements on {e.device}")
        self._check(self._lib.sfx_runner_phi_scalars(self._r, phi_bias.data_ptr(), phi_lambda.data_ptr()),
                    "sfx_runner_phi_scalars")
        self._phi_scalars = (phi_bias, phi_lambda)

    def phi_losses(self):
        """(loss, psi_loss, phi_loss, λ) of the last completed step that had an update (learned-φ schedules)."""
        out = (self._C.c_float * 4)()
        self._check(self._lib.sfx_runner_phi_losses(self._r, out), "sfx_runner_phi_losses")
        return tuple(float(v) for v in out)

    def close(self):
        if getattr(self, "_r", None):
            self._lib.sfx_runner_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_task(self, index: int):
        self._check(self._lib.sfx_runner_set_task(self._r, index), "sfx_runner_set_task")
        self.task_index = index

    def prefill(self, n: int):
        self._check(self._lib.sfx_runner_prefill(self._r, n), "sfx_runner_prefill")

    def run(self, n: int):
        self._check(self._lib.sfx_runner_run(self._r, n), "sfx_runner_run")

    def set_test_env(self, env):
        """sfx_runner_test_env: the test tasks' env of ``test_phase`` -- an object with ``reset(e) -> s0`` and
        ``step(e, a) -> (s1, phi, r, done)`` (numpy / floats; e is the test-task index), called through C
        callbacks like the training env's; None selects the built-in synthetic test tasks (the default).  The
        training env is never used for a test task."""
        C = self._C
        if env is None:
            self._check(self._lib.sfx_runner_test_env(self._r, None, None, None), "sfx_runner_test_env")
            self._test_cbs = None
            return
        from ._lib import ENV_RESET_FN, ENV_STEP_FN

        n_s, d = self.eng.n_s, self.eng.d

        def _reset(_ctx, e, s0):
            try:
                np.ctypeslib.as_array(s0, shape=(n_s,))[:] = np.asarray(env.reset(e), dtype=np.float32).reshape(n_s)
                return 0
            except Exception:  # reported as a failed phase by libsfx
                return 1

        def _step(_ctx, e, a, s1, phi, r, term):
            try:
                ns, ph, rr, tt = env.step(e, a)
                np.ctypeslib.as_array(s1, shape=(n_s,))[:] = np.asarray(ns, np.float32).reshape(n_s)
                if ph is None and self.schedule == "phi":  # phi_test_phase does not use the env's φ
                    np.ctypeslib.as_array(phi, shape=(d,))[:] = 0.0
                else:
                    np.ctypeslib.as_array(phi, shape=(d,))[:] = np.asarray(ph, np.float32).reshape(d)
                r[0] = float(rr)
                term[0] = 1 if tt else 0
                return 0
            except Exception:
                return 1

        cbs = (ENV_RESET_FN(_reset), ENV_STEP_FN(_step))
        self._check(self._lib.sfx_runner_test_env(self._r, C.cast(cbs[0], C.c_void_p), C.cast(cbs[1], C.c_void_p),
                                                  None), "sfx_runner_test_env")
        self._test_cbs = cbs  # kept alive while the runner may call them

    def test_phase(self, W, horizon=None, test_epsilon: float = 0.03, lr: float = 0.005, wd: float = 0.01,
                   explore=None, want_actions: bool = False):
        """sfx_runner_test_phase: ``[test_agent(task_e, e) for e in range(E)]`` of agents/sfdqn.py:139-166 with the
        E episodes in lockstep inside the runner (between runs).  W: a contiguous float32 device tensor
        [E, >= d], row e the test task's bias-free Linear(d, 1), updated in place.  horizon: steps per episode
        (default: the loop's episode_len, the reference's agent.T).  explore: None (the runner draws the
        ε-schedule from its own stream) or an int array [E, horizon] of explored actions, -1 = greedy
        (``draw_test_schedule`` keeps the reference's own ``random`` stream).  lr / wd: the SGD step of
        update_test_reward_mapper (:168-184).  Returns numpy ``(returns, loss_sums, steps)`` -- float64 [E],
        float64 [E], int64 [E] -- and, with want_actions, the taken actions int64 [E, horizon] (-1 once a row
        ended).  Training state is not touched: the next ``run`` continues as if no phase had run."""
        C, e = self._C, self.eng
        if not _is_f32_on(W, e.device, dim=2):
            raise ValueError(f"W: a contiguous float32 tensor [E, >= d] on {e.device}")
        E, stride = int(W.shape[0]), int(W.shape[1])
        horizon = int(self.episode_len if horizon is None else horizon)
        head = (self._r, E, horizon, float(test_epsilon), float(lr), float(wd), W.data_ptr(), stride)
        return _lockstep_call(C, self._check, self._lib.sfx_runner_test_phase, "sfx_runner_test_phase", head,
                              _explore_array(explore, (E, horizon)), E, horizon, want_actions)

    def tsf_test_phase(self, W, Omega, adam_state, opt_steps, hp, horizon=None, test_epsilon: float = 0.03,
                       explore=None, want_actions: bool = False):
        """sfx_runner_tsf_test_phase: ``[test_agent(task_e, e) for e in range(E)]`` of
        agents/tsfdqn_sequential.py:392-433 with the E episodes in lockstep inside the runner (schedule "tsf",
        between runs).  Row e of the contiguous float32 device tensors is test task e's state, updated in place:
        W [E, >= d] its reward weights, Omega [E, >= T] its ω, adam_state [E, >= 2(d + T)] the Adam moments
        (m_w, v_w, m_ω, v_ω; zeros before the first phase).  opt_steps: an int64 numpy array [E], the optimizer
        steps (= scheduler epochs) each task's optimizer has taken, advanced in place -- keep the four across
        phases, as the reference keeps every test task's optimizer and scheduler.  hp: a dict of gamma, beta,
        lasso, lr_w, wd_w, lr_omega, wd_omega, lr_omega_decay (ω's lr at epoch k is lr_omega (1 - decay)^k).
        explore: None (the runner draws the ε-schedule from its own stream) or an int array [E, horizon, 2] of
        the explored (a, a1), -1 = greedy (``draw_tsf_test_schedule`` keeps the reference's own ``random``
        stream).  Returns numpy ``(returns, losses, steps)`` -- float64 [E], float64 [E, 3] the sums of (loss,
        l2, l1), int64 [E] -- and, with want_actions, the taken (a, a1) int64 [E, horizon, 2] (-1 once a row
        ended).  Training state is not touched: the next ``run`` continues as if no phase had run."""
        from ._lib import TsfTestHP

        C, e = self._C, self.eng
        for name, t in (("W", W), ("Omega", Omega), ("adam_state", adam_state)):
            if not _is_f32_on(t, e.device, dim=2):
                raise ValueError(f"{name}: a contiguous float32 tensor [E, ...] on {e.device}")
        E = int(W.shape[0])
        if int(Omega.shape[0]) != E or int(adam_state.shape[0]) != E:
            raise ValueError(f"W, Omega and adam_state need the same number of rows (W has {E})")
        if not (isinstance(opt_steps, np.ndarray) and opt_steps.dtype == np.int64 and opt_steps.shape == (E,)
                and opt_steps.flags.c_contiguous and opt_steps.flags.writeable):
            raise ValueError(f"opt_steps: a writeable contiguous int64 numpy array [{E}]")
        missing = [k for k in TSF_TEST_HP if k not in hp]
        if missing or len(hp) != len(TSF_TEST_HP):
            raise ValueError(f"hp: a dict of exactly {TSF_TEST_HP}")
        chp = TsfTestHP(*(float(hp[k]) for k in TSF_TEST_HP))
        horizon = int(self.episode_len if horizon is None else horizon)
        opt = opt_steps if E else np.zeros(1, np.int64)
        head = (self._r, E, horizon, float(test_epsilon), C.byref(chp), W.data_ptr(), int(W.shape[1]), Omega.data_ptr(),
                int(Omega.shape[1]), adam_state.data_ptr(), int(adam_state.shape[1]), opt.ctypes.data_as(C.c_void_p))
        return _lockstep_call(C, self._check, self._lib.sfx_runner_tsf_test_phase, "sfx_runner_tsf_test_phase", head,
                              _explore_array(explore, (E, horizon, 2)), E, horizon, want_actions, (3,), (2,))

    def phi_test_phase(self, W, Wb, horizon=None, test_epsilon: float = 0.03, explore=None,
                       want_actions: bool = False):
        """sfx_runner_phi_test_phase: ``[test_agent(task_e, e) for e in range(E)]`` of agents/sfdqn_phi.py:234-261
        with the E episodes in lockstep inside the runner (schedule "phi", between runs).  W: a contiguous float32
        device tensor [E, >= d], row e the weight of test task e's biased Linear(d, 1); Wb: a contiguous float32
        device tensor of E elements, its bias; both are updated in place (update_test_reward_mapper :263-305, φ
        from the φ net on the device -- the test env's φ is not used and its ``step`` may return None for it).
        horizon: steps per episode (default: the loop's episode_len, the reference's agent.T).  explore: None (the
        runner draws the ε-schedule from its own stream) or an int array [E, horizon] of explored actions < A,
        -1 = greedy (``draw_test_schedule``: the draw is the SF agent's, :226-227).  Returns numpy ``(returns,
        loss_sums, steps)`` -- float64 [E], float64 [E], int64 [E] -- and, with want_actions, the taken actions
        int64 [E, horizon] (-1 once a row ended).  Training state is not touched: the next ``run`` continues as
        if no phase had run."""
        C, e = self._C, self.eng
        if not _is_f32_on(W, e.device, dim=2):
            raise ValueError(f"W: a contiguous float32 tensor [E, >= d] on {e.device}")
        E, stride = int(W.shape[0]), int(W.shape[1])
        if not (_is_f32_on(Wb, e.device) and Wb.numel() == E):
            raise ValueError(f"Wb: a contiguous float32 tensor of E = {E} elements on {e.device}")
        horizon = int(self.episode_len if horizon is None else horizon)
        ex = _explore_array(explore, (E, horizon))
        if ex is not None and ex.size and int(ex.max()) >= int(e.A):
            raise ValueError(f"explore: holds an action >= A = {int(e.A)}")
        head = (self._r, E, horizon, float(test_epsilon), W.data_ptr(), stride, Wb.data_ptr())
        return _lockstep_call(C, self._check, self._lib.sfx_runner_phi_test_phase, "sfx_runner_phi_test_phase", head,
                              ex, E, horizon, want_actions)

    def train(self, tasks, n_samples: int, W, n_test_ev: int = 1000, cycles_per_task: int = 1, **test_kwargs):
        """SFDQN.train's loop (agents/sfdqn.py:102-123) on the runner: for every cycle and every training task
        (``tasks``: the task indices, or their number), ``set_task`` and ``n_samples`` env steps, with a test phase
        (``test_phase(W, **test_kwargs)``; under schedule "tsf" ``tsf_test_phase(W, **test_kwargs)``, the other
        test-task state -- Omega, adam_state, opt_steps, hp -- among the keywords; under schedule "phi"
        ``phi_test_phase(W, **test_kwargs)``, the biases ``Wb`` among the keywords) after each training step t
        with ``t % n_test_ev == 0`` -- after step 1, step n_test_ev + 1, ...  Returns ``return_data``: per phase
        the float32 mean of the E returns, as ``torch.mean(torch.Tensor(Rs))`` gives.  All ``cycles_per_task``
        cycles run: the reference returns from inside its cycle loop after the first one, which is a
        bug and is not copied."""
        idx = list(range(tasks)) if isinstance(tasks, int) else [int(t) for t in tasks]
        return_data = []
        if self.schedule == "phi":
            phase = self.phi_test_phase
        else:
            phase = self.tsf_test_phase if self.schedule == "tsf" else self.test_phase
        for _ in range(int(cycles_per_task)):
            for index in idx:
                self.set_task(index)
                done = 0
                for t in test_phase_steps(n_samples, n_test_ev):
                    self.run(t + 1 - done)
                    done = t + 1
                    Rs = phase(W, **test_kwargs)[0]
                    return_data.append(torch.mean(torch.Tensor(Rs.tolist())).numpy()[()])
                self.run(n_samples - done)
        return return_data

    def action(self):
        out = (self._C.c_int64 * 3)()
        self._check(self._lib.sfx_runner_action(self._r, out), "sfx_runner_action")
        return int(out[0]), int(out[1])

    def warm(self):
        """Instantiate this schedule's step graphs (all span lengths, both slot parities) now."""
        self._check(self._lib.sfx_runner_warm(self._r), "sfx_runner_warm")

    def set_gate_timeout(self, seconds: float):
        """Bound of each step's gate wait; a step released later is cancelled and re-issued."""
        self._check(self._lib.sfx_runner_gate_timeout(self._r, float(seconds)), "sfx_runner_gate_timeout")

    def set_wait_timeout(self, seconds: float):
        """Bound of the host's wait on a step's result (sfx_runner_wait_timeout): past it the
        queued steps are cancelled and drained; a sharded step stuck in a collective gets its
        communicators aborted and the call raises instead of hanging."""
        self._check(self._lib.sfx_runner_wait_timeout(self._r, float(seconds)), "sfx_runner_wait_timeout")

    def stats(self) -> dict:
        C = self._C
        a, b, c, w, rt = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_double(), C.c_longlong()
        self._check(self._lib.sfx_runner_stats(self._r, C.byref(a), C.byref(b), C.byref(c), C.byref(w)),
                    "sfx_runner_stats")
        self._check(self._lib.sfx_runner_retried(self._r, C.byref(rt)), "sfx_runner_retried")
        rc, nf = C.c_longlong(), C.c_longlong()
        self._check(self._lib.sfx_runner_recomputed(self._r, C.byref(rc)), "sfx_runner_recomputed")
        self._check(self._lib.sfx_runner_nonfinite(self._r, C.byref(nf)), "sfx_runner_nonfinite")
        ps, ofs = C.c_longlong(), C.c_longlong()
        self._check(self._lib.sfx_runner_ahead_stats(self._r, C.byref(ps), C.byref(ofs)), "sfx_runner_ahead_stats")
        return {"env_steps": a.value, "prelaunched": b.value, "host_round_steps": c.value,
                "host_wait_us": round(w.value, 1), "retried": rt.value, "recomputed": rc.value,
                "nonfinite_steps": nf.value, "ahead_pre_steps": ps.value, "ahead_own_forward_steps": ofs.value}

    def gpi_counters(self) -> np.ndarray:
        T = self.eng.T_glob if self.schedule.startswith("sharded") else self.eng.T
        out = np.zeros(T * T, dtype=np.int64)
        self._check(self._lib.sfx_runner_gpi_counters(self._r, out.ctypes.data_as(self._C.POINTER(self._C.c_longlong))),
                    "sfx_runner_gpi_counters")
        return out.reshape(T, T)

    def record(self, capacity: int):
        self._check(self._lib.sfx_runner_record(self._r, capacity), "sfx_runner_record")

    def records(self) -> list:
        """Decoded input records: dict of numpy arrays + (task, have, c, a_greedy, a, terminal)."""
        C, e, B = self._C, self.eng, self.B
        shapes = {"s": ((B, e.n_s), np.float32), "s1": ((B, e.n_s), np.float32), "phi": ((B, e.d), np.float32),
                  "a": ((B,), np.int64), "gamma": ((B,), np.float32), "snext": ((e.n_s,), np.float32),
                  "phi1": ((e.d,), np.float32), "r1": ((1,), np.float32), "rb": ((B,), np.float32)}
        out = []
        for i in range(self._lib.sfx_runner_recorded(self._r)):
            buf = np.zeros(self.record_bytes, dtype=np.uint8)
            meta = (C.c_int64 * 6)()
            self._check(self._lib.sfx_runner_get_record(self._r, i, buf.ctypes.data_as(C.c_void_p), meta),
                        "sfx_runner_get_record")
            rec = {}
            for k, (shape, dt) in shapes.items():
                n = int(np.prod(shape)) * np.dtype(dt).itemsize
                rec[k] = buf[self.layout[k]:self.layout[k] + n].view(dt).reshape(shape).copy()
            rec.update(zip(("task", "have", "c", "a_greedy", "a_taken", "terminal"), (int(m) for m in meta)))
            out.append(rec)
        return out

