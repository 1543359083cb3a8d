"""Lockstep test-task rollouts: the test phase of agents/sfdqn.py, of the TSF agents and of agents/sfdqn_phi.py
with every test task stepped together (batched host envs).

The reference evaluates its test tasks one after the other (agents/sfdqn.py:111-115): each ``test_agent``
(:139-166) runs ``agent.T`` steps of its own env, choosing each action by GPI over all ψ heads under that task's
own reward model (``get_test_action``, :125-137) and fitting that model after every step
(``update_test_reward_mapper``, :168-184).  The ψ heads do not change during the test phase and every test task
owns its env and its reward model, so the E episodes are independent except for one shared thing: Python's
``random`` stream, from which each step draws ``random.random()`` (ε test) and, when exploring,
``random.randrange``.  The number of draws per step depends only on the first draw, never on the GPU's results,
so the whole schedule of draws is taken up front in the reference's order (task 0's steps, then task 1's, ...).
After that the E episodes run in lockstep: one launch set per step chooses all E greedy actions (row e under its
own reward model), the E envs step, and one launch set fits the E reward models on device copies of their rows,
written back into the users' modules when the phase ends -- the same arithmetic, the same draws, the same actions,
the same returns and log lines as the sequential loop, with one GPU round trip per step instead of E.  The E
losses of every step stay on the device and are read once (the reference's ``loss.item()`` is one device read per
task and step).  More test tasks than the engine takes in one call run as consecutive lockstep groups (the draws
are taken for all of them first).

Preconditions, checked before the first step (a phase never stops after it has moved an env or a reward model):
each test task owns its env and its random state (tasks/reacher.py: one bullet env with its own ``np_random`` per
task), since the lockstep order interleaves the tasks' env calls; and every episode runs the full ``agent.T``
steps (``fixed_horizon``: tasks/reacher.py:112 never ends one; other tasks declare ``episodes_never_end = True``,
or the caller passes ``episodes_end=False``).  An episode that ends early would shift every later task's draws, so
phases whose episodes may end run the reference's own sequential loop instead -- exact, one task after the other.
Should a task declared endless end anyway, it stops there (as the reference's ``break``) with a warning, and the
phase goes on with the remaining rows.

One loop (``_run_group``, under the header ``_phase``) serves the three kinds of phase; a kind supplies its engine
calls and its per-task bookkeeping:

SF (``test_tasks_lockstep``).  One ``sfx_test_actions`` launch set per step.  With agents/sfdqn.py's own reward
mapper (``device_reward_mapper``: a fresh SGD step of MSE(w(φ), r) per task and step) the E SGD steps of a
lockstep step run as ONE device launch (``sfx_test_reward_updates``).  Other mappers (the single-file sfdqn.py's
(w, Adam) pairs, user overrides) run as written, each right after its task's env step, and the step's losses are
read together.

TSF (``test_tasks_lockstep_tsf``; agents/tsfdqn_sequential.py:385-420, tsfdqn.py / tsfdqn_nf.py test_agent).
Each step draws twice (the action at s and the next action a1 at s1, both under the pre-update w and ω) and,
when ``total_training_steps % 1000 == 0``, the reward mapper's ``random.randint`` of its diagnostic print -- all
independent of the GPU, so again taken up front.  Per step: one ``sfx_tsf_test_actions`` launch set for the E
actions at s, the E env steps, one for the E actions at s1, one ``sfx_tsf_test_updates`` launch set fitting the E
(w, ω) pairs -- each task's own Adam step number, LR (its LambdaLR keeps decaying ω's) and r read per row -- then
each task's scheduler steps.  Console output: the same lines as the sequential loop over the bound reward mapper
(``sfx.dropin.bind.tsf_update_test_reward_mapper``, which shortens the reference's diagnostic block to one line),
but a step's lines are printed for all live tasks together, so across tasks their order interleaves where the
sequential loop prints task by task; the SF phase prints in the reference's order.

SF-φ (``test_tasks_lockstep_phi``; agents/sfdqn_phi.py:211-212 over test_agent :234-261).  The φ net and ψ heads
are read only, each test task owns its biased ``w_approx`` and the reward mapper builds a fresh Adam per step.
Here φ feeds ``w`` through Adam and ``w`` picks the next action, so the E-row kernels reproduce the one-row calls
bit for bit (csrc/sfx_phitest.h) and the phase follows the sequential trajectory exactly.  TSF-φ stays
sequential: all its test tasks write the one shared Ω.
"""
from __future__ import annotations

import random
import warnings
from typing import List, Sequence

import torch


def _draw_schedule(E: int, T: int, epsilon: float, n_actions: int) -> List[List[int]]:
    """The reference's random draws of E sequential test episodes of T steps (sfdqn.py:127-128):
    entry [e][j] is the explored action of task e's step j, or -1 for a greedy step."""
    sched = []
    for _ in range(E):
        row = []
        for _ in range(T):
            row.append(random.randrange(n_actions) if random.random() <= epsilon else -1)
        sched.append(row)
    return sched


def _tsf_draw_schedule(E: int, T: int, epsilon: float, n_actions: int, diag: bool) -> List[List[tuple]]:
    """The random draws of E sequential TSF test episodes (agents/tsfdqn_sequential.py:377-381,
    :399-402, :502): entry [e][j] = (action at s or -1 for greedy, action at s1 or -1, whether the
    diagnostic print fires)."""
    def one():
        return random.randrange(n_actions) if random.random() <= epsilon else -1

    sched = []
    for _ in range(E):
        row = []
        for _ in range(T):
            xa = one()
            xa1 = one()
            row.append((xa, xa1, diag and random.randint(1, 1000) < 10))
        sched.append(row)
    return sched


def fixed_horizon(test_tasks: Sequence, episodes_end=None) -> bool:
    """Whether every episode of ``test_tasks`` is known to run the full ``agent.T`` steps -- the
    lockstep precondition, decided BEFORE the first step (a phase never stops after it has moved
    an env or a reward model).  ``episodes_end=False`` is the caller's guarantee, ``True`` its
    denial; ``None`` asks the tasks: a task attribute ``episodes_never_end = True``, or the
    reference's Reacher (tasks/reacher.py:112 returns done = False on every step)."""
    if episodes_end is not None:
        return not episodes_end
    def never(task):
        if getattr(task, "episodes_never_end", False):
            return True
        cls = type(task)
        return cls.__name__ == "Reacher" and cls.__module__ in ("tasks.reacher", "reacher")
    return len(test_tasks) > 0 and all(never(t) for t in test_tasks)


def device_reward_mapper(agent) -> bool:
    """Whether the agent's ``update_test_reward_mapper`` is agents/sfdqn.py's own (:168-184: a fresh
    SGD(lr=0.005, weight_decay=0.01) step of MSE(w(φ), r) on a bias-free Linear(d, 1)), which the
    lockstep then runs on the device for all E test tasks in one launch (sfx_test_reward_updates).
    A subclass that overrides it, or an instance attribute, keeps the user's method."""
    if "update_test_reward_mapper" in vars(agent):
        return False
    f = getattr(type(agent), "update_test_reward_mapper", None)
    if f is None:
        return False
    if getattr(f, "__sfx_mapper__", None) == "sgd":
        return True
    return f.__module__ == "agents.sfdqn" and f.__qualname__ == "SFDQN.update_test_reward_mapper"


def phi_agent(agent) -> bool:
    """``agent`` is an SFDQN_PHI over sfx's DeepSF_PHI (agents/sfdqn_phi.py: biased reward models, no shared
    Ω), whose test phase ``test_tasks_lockstep_phi`` runs.  Told by the library alone: the agent gets its φ net
    (``agent.phi``) only in ``add_training_task`` (:136), inside ``train``."""
    return (not hasattr(agent, "omegas")
            and callable(getattr(getattr(agent, "sf", None), "phi_test_supported", None)))


def _rows(xs, dev):
    """[len(xs), n] float32 on ``dev``, one row per state, feature vector or weight in ``xs``."""
    return torch.cat([torch.as_tensor(x).to(dev, torch.float32).reshape(1, -1) for x in xs])


def _phase(make, agent, test_tasks, indices, episodes_end, sequential) -> List:
    """The header of the three public rollouts.  ``make(agent, test_tasks, idx)`` builds the phase's kind (below), or returns
    None where the kind refuses the agent's models; then, as when ``fixed_horizon`` fails, the sequential loop
    runs.  Otherwise: the draws for all E tasks, the groups of at most ``kind.cap`` tasks one after the other,
    and each task's log lines."""
    E = len(test_tasks)
    if E == 0:
        return []
    idx = list(range(E)) if indices is None else list(indices)
    kind = make(agent, test_tasks, idx) if fixed_horizon(test_tasks, episodes_end) else None
    if kind is None:
        seq = sequential or agent.test_agent
        return [seq(task, i) for i, task in zip(idx, test_tasks)]
    agent.sf._flush()
    kind.prepare()
    sched = kind.draw(E, int(agent.T))
    R, losses = [], []
    for lo in range(0, E, kind.cap):
        r_, l_ = _run_group(agent, kind, sched, lo, min(E, lo + kind.cap))
        R += r_
        losses += l_
    for e in range(E):
        kind.log(e, R[e], losses[e])
    return R


def _run_group(agent, kind, sched, lo, hi):
    """One lockstep group, the test tasks lo <= e < hi of the phase: (returns, per-task losses of the steps taken).
    ``kind.rows`` gives the group's per-task device tensors, row e - lo for task e.  While every task is live they
    and the step's slot of the loss block go to the kind's calls as they are; once a declared-endless episode has
    ended, the live rows are gathered for the call and scattered back after it."""
    E, T, dev, adev = hi - lo, int(agent.T), kind.eng.device, kind.adev
    test_tasks, rows = kind.tasks, kind.rows(lo, hi)
    L = kind.loss_block(T, E)  # [T, E, ...] on the device, read once; None: the kind reads a step's losses itself
    s_enc = {e: agent.encoding(test_tasks[e].initialize()) for e in range(lo, hi)}
    R, steps, losses = dict.fromkeys(s_enc, 0.0), dict.fromkeys(s_enc, 0), {e: [] for e in s_enc}
    live = list(s_enc)  # tasks whose episode is still running (all of them when the declaration holds)
    for j in range(T):
        part = len(live) < E
        sel = torch.tensor([e - lo for e in live], device=dev) if part else None
        sub = [t[sel].contiguous() for t in rows] if part else rows
        S = _rows([s_enc[e] for e in live], dev)
        greedy = kind.actions(j, live, S, sub)
        ended = []
        for k, e in enumerate(live):
            x = sched[e][j]
            a = torch.tensor(x).to(adev) if x >= 0 else greedy[k]
            s1, r, done = test_tasks[e].transition(a)
            s1 = agent.encoding(s1)
            kind.stepped(k, e, r, s_enc[e], a, s1)
            s_enc[e] = s1
            R[e] += r
            steps[e] += 1
            if done and j + 1 < T:
                warnings.warn(f"sfx.lockstep: test task {kind.idx[e]} ended at step {j + 1} of {T} although its episodes "
                              "were declared never to end; it stops there, and the random draws of the later test "
                              "tasks no longer follow the sequential loop's order", RuntimeWarning, stacklevel=4)
                ended.append(e)
        Lj = kind.update(S, [s_enc[e] for e in live], sub, None if part or L is None else L[j])
        if L is None:
            for e, v in zip(live, Lj):
                losses[e].append(v)
        elif part:
            for t, tl in zip(rows, sub):
                t[sel] = tl
            L[j, sel] = Lj
        live = [e for e in live if e not in ended]
        if not live:
            break
    with torch.no_grad():
        for e in range(lo, hi):
            kind.write(e, [t[e - lo] for t in rows])
    if L is not None:
        Lh = L.cpu().tolist()  # one device read for the group's losses
        losses = {e: [Lh[j][e - lo] for j in range(steps[e])] for e in s_enc}
    return list(R.values()), list(losses.values())


class _Kind:
    """What a kind of test phase adds to ``_phase`` and ``_run_group``; ``e`` is a task's position in the phase,
    ``k`` its position among the step's live tasks (the row of ``S`` and of the gathered ``rows``).  A kind has
    ``eng``, ``cap`` (the most tasks of one group), ``rows(lo, hi)``, ``actions(j, live, S, rows)`` -> the live
    tasks' greedy actions, ``stepped(k, e, r, s, a, s1)`` right after task e's env step,
    ``update(S, s1, rows, out)`` -> the live rows' losses (in ``out`` when given) and ``write(e, row)``: task e's
    rows into the user's modules.  The members below are the ones most kinds share."""
    loss_shape = ()

    def __init__(self, agent, tasks, idx, ws, eng, cap):
        self.agent, self.tasks, self.idx, self.ws, self.eng, self.cap = agent, tasks, idx, ws, eng, cap
        self.adev = getattr(agent, "device", None) or agent.sf._out_device()  # where the actions go to the envs

    def prepare(self):
        pass

    def draw(self, E, T):
        self.sched = _draw_schedule(E, T, float(self.agent.test_epsilon), int(self.agent.n_actions))
        return self.sched

    def loss_block(self, T, E):
        return torch.zeros(T, E, *self.loss_shape, device=self.eng.device)

    def log(self, e, R, losses):
        acc = 0  # accum_loss of test_agent: a python sum of .item()
        for v in losses:
            acc += v
        agent = self.agent
        agent.logger.log_target_error_progress(agent.get_target_reward_mapper_error(R, acc, self.idx[e], int(agent.T)))


class _SFDevice(_Kind):
    """agents/sfdqn.py with its own reward mapper: rows (W,), the E SGD steps of a step in one launch."""

    def rows(self, lo, hi):
        return [_rows([w.weight.detach() for w in self.ws[lo:hi]], self.eng.device).contiguous()]

    def actions(self, j, live, S, rows):
        self.phis, self.rs = [], []
        return self.eng.test_actions(S, rows[0])[:, 1].unbind()

    def stepped(self, k, e, r, s, a, s1):
        self.phis.append(self.tasks[e].features(s, a, s1))
        self.rs.append(float(r))

    def update(self, S, s1, rows, out):
        return self.eng.test_reward_updates(_rows(self.phis, self.eng.device), torch.tensor(self.rs, dtype=torch.float32),
                                            rows[0], losses=out)

    def write(self, e, row):
        w = self.ws[e].weight
        w.copy_(row[0].view_as(w))


class _SFUser(_Kind):
    """A user's reward mapper, or the single-file sfdqn.py's (w_approx, optim) pairs with the optimizer passed to
    update_test_reward_mapper (sfdqn.py:652, :723): no device rows; W is read from the users' modules at every
    step, and the mapper runs as written between the tasks' env steps."""

    def rows(self, lo, hi):
        return []

    def loss_block(self, T, E):
        return None

    def actions(self, j, live, S, rows):
        self.losses = []
        W = _rows([self.ws[e][0].weight.detach() for e in live], self.eng.device)
        return self.eng.test_actions(S, W)[:, 1].unbind()

    def stepped(self, k, e, r, s, a, s1):
        self.losses.append(self.agent.update_test_reward_mapper(*self.ws[e], self.tasks[e], r, s, a, s1))

    def update(self, S, s1, rows, out):
        return torch.stack([l.detach().reshape(()) for l in self.losses]).tolist()

    def write(self, e, row):
        pass


class _TSF(_Kind):
    """The TSF agents: rows (W, Ω, Adam moments), three losses; ``agent.test_tasks_weights[i]`` = (w_approx,
    optim, scheduler) and ``agent.omegas[i]`` as the reference's train builds them (:320-348).  The moments and
    step counts are kept where the per-call binding keeps them (``sf._test_state``)."""
    loss_shape = (3,)

    def prepare(self):
        from sfx.dropin.bind import prints_phi_shape

        agent = self.agent
        sync = getattr(agent.sf, "sync_tsf_modules", None)  # what the bound test_agent does first
        if sync is not None:
            sync()
        if getattr(agent, "h_function", None) is None:
            raise Exception('Affine Function (h) is not initialized')
        self.ws = [agent.test_tasks_weights[i] for i in self.idx]
        self.omegas = [agent.omegas[i] for i in self.idx]
        for _, optim, _ in self.ws:
            for grp in optim.param_groups[:2]:
                if tuple(grp.get("betas", (0.9, 0.999))) != (0.9, 0.999) or grp.get("eps", 1e-8) != 1e-8:
                    raise NotImplementedError("sfx: the test reward mapper's Adam runs with betas (0.9, 0.999), eps 1e-8")
        self.phi_line, self.states = prints_phi_shape(agent), {}

    def draw(self, E, T):
        agent = self.agent
        self.sched = _tsf_draw_schedule(E, T, float(agent.test_epsilon), int(agent.n_actions),
                                        agent.total_training_steps % 1000 == 0)
        return [[x[0] for x in row] for row in self.sched]

    def rows(self, lo, hi):
        sf, dev = self.agent.sf, self.eng.device
        for e in range(lo, hi):
            st = sf._test_state.get(self.omegas[e])
            if st is None:
                st = sf._test_state[self.omegas[e]] = [torch.zeros(2 * (int(sf.n_features) + int(sf.n_tasks)), device=dev), 0]
            self.states[e] = st
        flat = lambda x: x.detach().reshape(-1).to(dev, torch.float32)  # noqa: E731
        return [torch.stack([flat(w.weight) for w, _, _ in self.ws[lo:hi]]).contiguous(),
                torch.stack([flat(o) for o in self.omegas[lo:hi]]).contiguous(),
                torch.stack([self.states[e][0] for e in range(lo, hi)]).contiguous()]

    def actions(self, j, live, S, rows):
        self.j, self.live = j, live
        self.acts, self.phis, self.rowp = [], [], []
        return self.eng.tsf_test_actions(S, rows[0], rows[1]).to(self.adev).unbind()

    def stepped(self, k, e, r, s, a, s1):
        dev = self.eng.device
        phi = torch.as_tensor(self.tasks[e].features(s, a, s1))
        self.phis.append(phi)
        self.acts.append(a.reshape(()).to(dev, torch.long))
        st = self.states[e]
        st[1] += 1
        gw, go = self.ws[e][1].param_groups[:2]
        self.rowp.append([float(r), gw['lr'], gw['weight_decay'], go['lr'], go['weight_decay'], float(st[1])])

    def update(self, S, s1, rows, out):
        agent, eng, j, live = self.agent, self.eng, self.j, self.live
        dev, hp, (W, Om, M) = eng.device, agent.hyperparameters, rows
        S1 = _rows(s1, dev)
        A1 = eng.tsf_test_actions(S1, W, Om)
        ex = [(k, self.sched[e][j][1]) for k, e in enumerate(live) if self.sched[e][j][1] >= 0]
        if ex:
            A1[[k for k, _ in ex]] = torch.tensor([x for _, x in ex], dtype=torch.long).to(dev)
        rowp = torch.tensor(self.rowp, dtype=torch.float32).to(dev)
        Lj = eng.tsf_test_updates(S, S1, torch.stack(self.acts), A1, _rows(self.phis, dev), W, Om, M, rowp, agent.gamma,
                                  hp['beta_loss_coefficient'], hp['omegas_l1_coefficient'], losses=out)
        if self.phi_line:  # agents/tsfdqn_sequential.py:443, once per task and step (bind.prints_phi_shape)
            for phi in self.phis:
                print(f'Phi values {phi.shape}')
        printed = [(k, e) for k, e in enumerate(live) if self.sched[e][j][2]]
        if printed:  # the binding's diagnostic print (bind.tsf_update_test_reward_mapper), over the written-back rows
            with torch.no_grad():
                for k, e in printed:
                    self.write(e, [W[k], Om[k], M[k]])
            for _, e in printed:
                print(f'Target Task {self.tasks[e]} omegas {self.omegas[e].detach()} weights '
                      f'{self.ws[e][0].weight.detach()}')
        for e in live:
            self.ws[e][2].step()
        return Lj

    def write(self, e, row):
        w = self.ws[e][0].weight
        w.copy_(row[0].view_as(w))
        self.omegas[e].copy_(row[1].view_as(self.omegas[e]))
        self.states[e][0].copy_(row[2])

    def log(self, e, R, losses):
        agent = self.agent
        if agent.total_training_steps % 5000 != 0:
            return
        acc = [0, 0, 0]  # accum_loss, total_phi_loss (l2), total_psi_loss (l1): python sums of .item()
        for row in losses:
            for k in range(3):
                acc[k] += row[k]
        agent.logger.log_target_error_progress(agent.get_target_reward_mapper_error(
            R, acc[0], acc[1], acc[2], self.idx[e], agent.hyperparameters['beta_loss_coefficient'], int(agent.T)))
        agent.logger.log_omegas_learning_rate(self.ws[e][1].param_groups[1]['lr'], self.idx[e],
                                              agent.total_training_steps)


class _Phi(_Kind):
    """agents/sfdqn_phi.py: rows (weight, bias) of the biased reward models; the step's E actions are read once
    and go to the update as Python ints."""

    def rows(self, lo, hi):
        dev = self.eng.device
        return [_rows([w.weight.detach() for w in self.ws[lo:hi]], dev).contiguous(),
                torch.cat([w.bias.detach().to(dev, torch.float32).reshape(1) for w in self.ws[lo:hi]]).contiguous()]

    def actions(self, j, live, S, rows):
        self.j, self.acts, self.rs = j, [], []
        greedy = self.eng.phi_test_actions(S, rows[0], rows[1])[:, 1]
        self.picked = greedy.tolist()  # the step's one read of the E actions
        return greedy.to(self.adev).unbind()

    def stepped(self, k, e, r, s, a, s1):
        x = self.sched[e][self.j]
        self.acts.append(x if x >= 0 else self.picked[k])
        self.rs.append(float(r))

    def update(self, S, s1, rows, out):
        dev = self.eng.device
        return self.eng.phi_test_updates(S, torch.tensor(self.acts, dtype=torch.long),
                                         torch.tensor(self.rs, dtype=torch.float32),
                                         _rows(s1, dev), rows[0], rows[1], losses=out)

    def write(self, e, row):
        w = self.ws[e]
        w.weight.copy_(row[0].view_as(w.weight))
        w.bias.copy_(row[1].view_as(w.bias))


def _sf_kind(agent, tasks, idx):
    ws = [agent.test_tasks_weights[i] for i in idx]
    eng = agent.sf._engine(len(idx))  # asked for all E rows: one group
    if isinstance(ws[0], tuple) or not device_reward_mapper(agent):
        return _SFUser(agent, tasks, idx, [w if isinstance(w, tuple) else (w,) for w in ws], eng, len(idx))
    return _SFDevice(agent, tasks, idx, ws, eng, len(idx))


def _tsf_kind(agent, tasks, idx):
    eng = agent.sf._engine(1)
    return _TSF(agent, tasks, idx, None, eng, int(eng.max_batch))


def _phi_kind(agent, tasks, idx):
    """None (the sequential loop) unless the library takes every reward model and the φ net."""
    sf, phi_model = agent.sf, agent.phi[0][0]
    ws = [agent.test_tasks_weights[i] for i in idx]
    if not all(sf.phi_test_supported(phi_model, w) for w in ws):
        return None
    eng = sf._phi_engine(phi_model, 1)  # loads the φ net on first use, as the bound update_test_reward_mapper
    return _Phi(agent, tasks, idx, ws, eng, max(1, min(int(eng.PHI_ROWS), int(eng.max_batch))))


def test_tasks_lockstep(agent, test_tasks: Sequence, indices: Sequence[int] = None, *, episodes_end=None,
                        sequential=None) -> List:
    """``[agent.test_agent(task, i) for i, task in enumerate(test_tasks)]`` of agents/sfdqn.py (or of the
    single-file sfdqn.py, :665-721) with the episodes in lockstep.  ``agent`` is the user's SFDQN over ``sfx``'s
    drop-in ``DeepSF`` (``agent.sf``); returns the E returns R (as test_agent does).

    Lockstep runs only when ``fixed_horizon(test_tasks, episodes_end)`` holds; otherwise the reference's own
    sequential loop runs (``sequential(task, index)``, default ``agent.test_agent``), which is exact for episodes
    that end early.  With agents/sfdqn.py's reward mapper (``device_reward_mapper``) the E SGD steps of a lockstep
    step are one device launch and the losses one device read per phase; other mappers run as the user wrote
    them."""
    return _phase(_sf_kind, agent, test_tasks, indices, episodes_end, sequential)


def test_tasks_lockstep_tsf(agent, test_tasks: Sequence, indices: Sequence[int] = None, *, episodes_end=None,
                            sequential=None) -> List:
    """The same of the TSF agents (agents/tsfdqn_sequential.py:385-420).  ``agent`` is the user's TSFDQN over sfx's
    drop-in DeepTSF; w_approx and ω are updated in place, the Adam moments kept in ``sf._test_state``; returns the
    E returns.  More test tasks than the engine's max_batch run as consecutive lockstep groups.  The fallback to
    the sequential loop is ``test_tasks_lockstep``'s."""
    return _phase(_tsf_kind, agent, test_tasks, indices, episodes_end, sequential)


def test_tasks_lockstep_phi(agent, test_tasks: Sequence, indices: Sequence[int] = None, *, episodes_end=None,
                            sequential=None) -> List:
    """The same of agents/sfdqn_phi.py (:211-212 over test_agent :234-261).  ``agent`` is the user's SFDQN_PHI over
    sfx's drop-in DeepSF_PHI; ``agent.test_tasks_weights[i]`` the test task's nn.Linear(d, 1) with bias, updated
    in place.  Per step: one ``sfx_phi_test_actions`` launch set and one read of the E greedy actions, the E env
    steps, one ``sfx_phi_test_updates`` launch set (the φ net streamed once for the E transitions).  Every row of
    both is bit for bit the one-row call's result, so the actions, returns, reward models, log lines and the
    random state are the sequential loop's.  More than the engine's ``PHI_ROWS`` test tasks run as consecutive
    groups.  The sequential loop runs when ``fixed_horizon`` fails or ``sf.phi_test_supported`` refuses a model."""
    return _phase(_phi_kind, agent, test_tasks, indices, episodes_end, sequential)



def enable(agent, episodes_end=None) -> None:
    """Bind lockstep test rollouts into an SFDQN or TSFDQN instance without touching its code: ``train``
    records its ``test_tasks``; the first ``test_agent`` call of a test phase (test_index 0) runs
    all of them in lockstep and the later calls of that phase return the stored returns, so the
    reference's loop (agents/sfdqn.py:111-120) sees the same values in the same order.  A
    ``test_agent`` call outside that pattern runs its one task alone (E = 1, sequential
    semantics).  ``episodes_end`` is passed to ``fixed_horizon``: phases whose episodes may end
    early run the agent's own sequential ``test_agent``."""
    train, state = agent.train, {"tasks": None, "R": None}
    own = agent.test_agent  # the user's sequential loop: the fallback

    def rollout(*args, **kwargs):
        # chosen per call: the TSF agents (test_tasks_weights of (w_approx, optim, scheduler) and per-task ω),
        # SFDQN_PHI over sfx's DeepSF_PHI (a learned φ, biased reward models), or SFDQN
        if hasattr(agent, "omegas"):
            return test_tasks_lockstep_tsf(*args, **kwargs)
        return (test_tasks_lockstep_phi if phi_agent(agent) else test_tasks_lockstep)(*args, **kwargs)

    def train_recording(*args, **kwargs):
        tasks = kwargs.get("test_tasks", args[4] if len(args) > 4 else [])
        state["tasks"], state["R"] = list(tasks), None
        return train(*args, **kwargs)

    def test_agent(task, test_index):
        tasks = state["tasks"]
        if tasks and test_index < len(tasks) and tasks[test_index] is task:
            if test_index == 0 or state["R"] is None:
                state["R"] = rollout(agent, tasks, episodes_end=episodes_end, sequential=own)
            return state["R"][test_index]
        return rollout(agent, [task], [test_index], episodes_end=episodes_end, sequential=own)[0]

    agent.train = train_recording
    agent.test_agent = test_agent
