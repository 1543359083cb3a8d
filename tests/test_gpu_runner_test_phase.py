"""The native runner's test phase (sfx_runner_test_env / sfx_runner_test_phase, NativeEnvLoop.test_phase and
.train): E test episodes of agents/sfdqn.py:139-166 stepped in lockstep inside the runner.

  1. bit for bit against a Python loop of SFEngine.test_actions + SFEngine.test_reward_updates;
  2. against the CPU oracle (oracle.ref_cpu psi_all / gpi_w / sf_test_reward_update);
  3. rows whose env reports done stop after that step's update;
  4. training is untouched by a phase (heads, Adam state, w, target counters, GPI counters, actions);
  5. a second identical phase captures no graph; built-in tasks and schedule are seed-deterministic;
  6. refusals name the limit and leave the runner usable.
"""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.conftest import gpu_available
from tests.test_gpu_engine import rel_close

pytestmark = pytest.mark.gpu

N_S, H, A = 6, 64, 9
HORIZON = 9
ORACLE_SEED = 16  # test 2's env / W / schedule seed: its top-2 gap precondition holds (asserted there)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


class DetEnv:
    """Deterministic test tasks: task e's stream depends only on (seed, e) and the actions it was given.
    done_at: {e: step index at which task e reports done}."""

    def __init__(self, E, d, seed, done_at=None):
        self.E, self.d, self.seed, self.done_at = E, d, seed, dict(done_at or {})
        self.rng = [None] * E
        self.t = [0] * E

    def reset(self, e):
        self.rng[e] = np.random.default_rng([self.seed, e])
        self.t[e] = 0
        return self.rng[e].standard_normal(N_S, dtype=np.float32)

    def step(self, e, a):
        g = self.rng[e]
        s1 = g.standard_normal(N_S, dtype=np.float32) + np.float32(0.05 * a)
        phi = g.random(self.d, dtype=np.float32)
        r = np.float32(phi[e % self.d] + np.float32(0.125) * np.float32(a % 3))
        done = self.done_at.get(e) == self.t[e]
        self.t[e] += 1
        return s1, phi, float(r), done


def heads_of(T, d, seed=0):
    from sfx.init import reference_heads

    return reference_heads(T, N_S, H, A, d, ("relu", "relu"), seed=seed)[0]


def make_engine(T, d, seed=0):
    from sfx.engine import SFEngine
    from sfx.init import reference_heads

    online, w = reference_heads(T, N_S, H, A, d, ("relu", "relu"), seed=seed)
    eng = SFEngine(T, N_S, H, A, d, ("relu", "relu"), max_batch=16)
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    eng.set_target_update_ev(7)
    for t in range(T):
        eng.load_head(t, online[t], 0)
        eng.load_head(t, online[t], 1)
        eng.load_w(t, w[t])
    return eng


def initial_W(E, d, stride, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    W = torch.zeros(E, stride)
    W[:, :d] = torch.empty(E, d).uniform_(-1.0, 1.0, generator=g)
    return W


def schedule(E, horizon, eps, seed):
    g = np.random.default_rng(500 + seed)
    u = g.random((E, horizon))
    x = g.integers(0, A, (E, horizon))
    return np.where(u <= eps, x, -1).astype(np.int32)


def python_phase(eng, env, W, d, explore, horizon):
    """The phase as a Python loop over the existing calls: one test_actions and one test_reward_updates per
    lockstep step; a row that ended keeps its W (restored after the E-row launch), return, loss and steps."""
    E = W.shape[0]
    S = np.stack([env.reset(e) for e in range(E)])
    live = [True] * E
    ret, loss = np.zeros(E), np.zeros(E)
    steps = np.zeros(E, np.int64)
    acts = np.full((E, horizon), -1, np.int64)
    Wv = W[:, :d]
    for j in range(horizon):
        sel = eng.test_actions(torch.from_numpy(S).to(eng.device), Wv.contiguous()).cpu().numpy()
        PHI, r = np.zeros((E, d), np.float32), np.zeros(E, np.float32)
        took = list(live)
        for e in range(E):
            if not live[e]:
                continue
            a = int(explore[e, j]) if explore[e, j] >= 0 else int(sel[e, 1])
            s1, phi, rr, done = env.step(e, a)
            S[e], PHI[e], r[e] = s1, phi, np.float32(rr)
            acts[e, j] = a
            ret[e] += float(r[e])
            steps[e] += 1
            live[e] = not done
        keep = W.clone()
        lo = eng.test_reward_updates(torch.from_numpy(PHI).to(eng.device), torch.from_numpy(r).to(eng.device), Wv).cpu()
        for e in range(E):
            if took[e]:
                loss[e] += float(lo[e])
            else:
                W[e] = keep[e]
        if not any(live):
            break
    return ret, loss, steps, acts


def native_phase(eng, E, d, stride, seed, done_at=None, horizon=HORIZON, eps=0.3):
    from sfx.runner import NativeEnvLoop

    loop = NativeEnvLoop(eng, batch=16, capacity=100, episode_len=horizon, seed=3)
    try:
        loop.set_test_env(DetEnv(E, d, seed, done_at))
        W = initial_W(E, d, stride, seed).to(eng.device)
        ret, loss, steps, acts = loop.test_phase(W, explore=schedule(E, horizon, eps, seed), want_actions=True)
        return ret.copy(), loss.copy(), steps.copy(), acts.copy(), W.cpu()
    finally:
        loop.close()


@pytest.fixture(scope="module")
def base_5_8():
    """The phase of (E, d, w_stride) = (5, 8, 8) without early ends, computed once (tests 1 and 3)."""
    if not gpu_available():
        pytest.skip("no HIP device")
    eng = make_engine(4, 8)
    try:
        return native_phase(eng, 5, 8, 8, seed=1)
    finally:
        eng.close()


@pytest.mark.parametrize("E,d,stride", [(5, 8, 8), (17, 20, 24), (40, 12, 12)])
def test_phase_bit_for_bit_against_existing_calls(E, d, stride, base_5_8):
    """A ragged tile; a row past the first 16-row tile with stride > d; more than max_batch rows (the forward
    is chunked)."""
    T = {5: 4, 17: 3, 40: 6}[E]
    eng = make_engine(T, d)
    try:
        got = base_5_8 if E == 5 else native_phase(eng, E, d, stride, seed=1)
        W = initial_W(E, d, stride, 1).to(eng.device)
        ret, loss, steps, acts = python_phase(eng, DetEnv(E, d, 1), W, d, schedule(E, HORIZON, 0.3, 1), HORIZON)
        assert (got[3] >= 0).all() and (got[3] < A).all()
        assert np.array_equal(got[3], acts)
        assert torch.equal(got[4], W.cpu())
        assert got[1].tolist() == loss.tolist()
        assert got[0].tolist() == ret.tolist()
        assert got[2].tolist() == [HORIZON] * E and steps.tolist() == [HORIZON] * E
        assert (schedule(E, HORIZON, 0.3, 1) >= 0).any() and (schedule(E, HORIZON, 0.3, 1) < 0).any()
    finally:
        eng.close()


def oracle_phase(online, spec, env, W, explore, horizon):
    """The phase on the CPU: ψ of every head, GPI under each row's own w, the reference's SGD by autograd.
    Returns (actions, loss sums, the smallest top-2 gap of a greedy step relative to the largest |q|)."""
    E = W.shape[0]
    S = torch.from_numpy(np.stack([env.reset(e) for e in range(E)]))
    acts = np.full((E, horizon), -1, np.int64)
    loss = np.zeros(E)
    min_gap = float("inf")
    for j in range(horizon):
        psi = R.psi_all(online, spec, S)
        for e in range(E):
            q, task = R.gpi_w(psi[e:e + 1], W[e])
            c = int(task[0])
            a = int(torch.argmax(q[0, c, :]))
            if explore[e, j] >= 0:
                a = int(explore[e, j])
            else:  # the values that decide c (the heads' maxima) and a (row c of q)
                scale = float(q.abs().max())
                for v in (q[0].max(dim=1).values, q[0, c, :]):
                    top = torch.topk(v, 2).values
                    min_gap = min(min_gap, float(top[0] - top[1]) / scale)
            s1, phi, r, _ = env.step(e, a)
            loss[e] += R.sf_test_reward_update(W[e], torch.from_numpy(phi), float(np.float32(r)))
            S[e] = torch.from_numpy(s1)
            acts[e, j] = a
    return acts, loss, min_gap


def test_phase_against_oracle():
    E, d, T = 5, 8, 4
    spec = R.Spec(N_S, H, A, d, ("relu", "relu"))
    explore = schedule(E, HORIZON, 0.3, ORACLE_SEED)
    W_ref = initial_W(E, d, d, ORACLE_SEED)
    acts, loss, min_gap = oracle_phase(heads_of(T, d), spec, DetEnv(E, d, ORACLE_SEED), W_ref, explore, HORIZON)
    # the test's own precondition: no greedy step of the oracle is a near tie
    assert min_gap > 1e-3, min_gap
    eng = make_engine(T, d)
    try:
        got = native_phase(eng, E, d, d, seed=ORACLE_SEED)
    finally:
        eng.close()
    assert np.array_equal(got[3], acts)  # every step, none excluded
    rel_close(got[4], W_ref, rtol=1e-4, atol=1e-7)
    rel_close(got[1], loss, rtol=1e-4, atol=1e-7)
    assert got[2].tolist() == [HORIZON] * E


def test_phase_early_end(base_5_8):
    E, d = 5, 8
    done_at = {2: 3, 0: HORIZON - 1}
    eng = make_engine(4, d)
    try:
        ret, loss, steps, acts, W = native_phase(eng, E, d, d, seed=1, done_at=done_at)
        Wp = initial_W(E, d, d, 1).to(eng.device)
        pret, ploss, psteps, pacts = python_phase(eng, DetEnv(E, d, 1, done_at), Wp, d, schedule(E, HORIZON, 0.3, 1),
                                                  HORIZON)
    finally:
        eng.close()
    assert steps.tolist() == [HORIZON, HORIZON, 4, HORIZON, HORIZON]
    assert psteps[2] == 4
    assert torch.equal(W[2], Wp.cpu()[2])  # the Python loop's W after 4 updates
    assert (acts[2, 4:] == -1).all() and (acts[2, :4] >= 0).all()
    assert np.array_equal(acts[2], pacts[2])
    assert loss[2] == ploss[2] and ret[2] == pret[2]
    assert not torch.equal(W[2], base_5_8[4][2])  # 4 updates, not 9
    for e in (0, 1, 3, 4):  # row 0 ends at the last step: nothing of it changes
        assert torch.equal(W[e], base_5_8[4][e])
        assert np.array_equal(acts[e], base_5_8[3][e])
        assert ret[e] == base_5_8[0][e] and loss[e] == base_5_8[1][e]


def _training_state(eng, loop, T):
    heads = [torch.stack([eng.get_head(t, which) for t in range(T)]) for which in (0, 1)]
    adam = [eng.get_adam(t) for t in range(T)]
    w = [eng.get_w(t) for t in range(T)]
    return {"heads": heads, "m": torch.stack([a[0] for a in adam]), "v": torch.stack([a[1] for a in adam]),
            "steps": [a[2] for a in adam], "w": torch.stack([torch.cat([x.reshape(-1) for x in ww]) for ww in w]),
            "since": [eng.since_target(t) for t in range(T)], "gpi": loop.gpi_counters()}


def _same_state(a, b):
    for x, y in zip(a["heads"], b["heads"]):
        assert torch.equal(x, y)
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]) and a["steps"] == b["steps"]
    assert torch.equal(a["w"], b["w"])
    assert a["since"] == b["since"]
    assert np.array_equal(a["gpi"], b["gpi"])


@pytest.mark.parametrize("sched", ["all", "active"])
def test_training_untouched_by_a_phase(sched):
    from sfx.runner import NativeEnvLoop

    T, d, E = 3, 8, 5

    def run(with_phase):
        eng = make_engine(T, d)
        loop = NativeEnvLoop(eng, batch=16, capacity=200, gamma=0.9, epsilon=0.3, alpha_w=0.05, episode_len=7, seed=5,
                             schedule=sched)
        try:
            loop.prefill(20)
            loop.set_task(0)
            loop.run(30)
            if with_phase:
                W = initial_W(E, d, d, 2).to(eng.device)
                _, _, steps = loop.test_phase(W, horizon=HORIZON)
                assert steps.tolist() == [HORIZON] * E
            loop.record(40)
            loop.run(30)
            loop.set_task(1)
            loop.run(10)
            recs = loop.records()
            assert len(recs) == 40
            st = _training_state(eng, loop, T)
            st["actions"] = [(r["task"], r["c"], r["a_greedy"], r["a_taken"]) for r in recs]
            return st
        finally:
            loop.close()
            eng.close()

    a, b = run(True), run(False)
    _same_state(a, b)
    assert a["actions"] == b["actions"]
    assert sum(a["steps"]) > 0  # the runs did train


def test_train_loop_phases_and_heads():
    """NativeEnvLoop.train: n_test_ev = 10 over 25 steps evaluates after steps 1, 11 and 21 of every task and
    leaves the heads of the same runs without phases."""
    from sfx.runner import NativeEnvLoop, test_phase_steps

    T, d, E, n = 3, 8, 5, 25
    out = []
    for with_phase in (True, False):
        eng = make_engine(T, d)
        loop = NativeEnvLoop(eng, batch=16, capacity=200, epsilon=0.3, alpha_w=0.05, episode_len=7, seed=9)
        try:
            loop.prefill(20)
            if with_phase:
                W = initial_W(E, d, d, 4).to(eng.device)
                data = loop.train([0, 2], n, W, n_test_ev=10, horizon=6)
                assert len(data) == 3 * 2 and all(isinstance(v, np.float32) and np.isfinite(v) for v in data)
                assert not torch.equal(W.cpu(), initial_W(E, d, d, 4))
            else:
                for task in (0, 2):
                    loop.set_task(task)
                    done = 0
                    for t in test_phase_steps(n, 10):
                        loop.run(t + 1 - done)
                        done = t + 1
                    loop.run(n - done)
            assert loop.stats()["env_steps"] == 2 * n
            out.append(_training_state(eng, loop, T))
        finally:
            loop.close()
            eng.close()
    _same_state(out[0], out[1])


def test_graph_reuse_and_determinism():
    from sfx.runner import NativeEnvLoop

    T, d, E = 4, 8, 5

    def builtin(seed, phases=1):
        eng = make_engine(T, d)
        loop = NativeEnvLoop(eng, batch=16, capacity=100, episode_len=HORIZON, seed=seed)
        try:
            W = initial_W(E, d, d, 6).to(eng.device)
            caps = []
            for _ in range(phases):
                W.copy_(initial_W(E, d, d, 6))
                ret, loss, steps, acts = loop.test_phase(W, test_epsilon=0.3, want_actions=True)
                caps.append(eng.graph_stats()["captures"])
            return ret.copy(), acts.copy(), W.cpu(), caps
        finally:
            loop.close()
            eng.close()

    # two phases with the same arguments: the second captures nothing (at most three graphs in the first)
    *_, caps = builtin(21, phases=2)
    assert caps[1] == caps[0] and 1 <= caps[0] <= 3
    r1, a1, w1, _ = builtin(21)
    r2, a2, w2, _ = builtin(21)
    assert r1.tolist() == r2.tolist() and np.array_equal(a1, a2) and torch.equal(w1, w2)
    r3, a3, _, _ = builtin(22)
    assert not np.array_equal(a1, a3) and r1.tolist() != r3.tolist()
    assert (a1 >= 0).all() and (a1 < A).all()


def test_refusals_leave_the_runner_usable():
    from sfx import _lib
    from sfx.runner import NativeEnvLoop
    from sfx.pretrain import PreEngine

    T, d, E = 3, 8, 5
    eng = make_engine(T, d)
    loop = NativeEnvLoop(eng, batch=16, capacity=100, episode_len=HORIZON, seed=2)
    try:
        W = initial_W(E, d, d, 7).to(eng.device)

        def refused(code, word, **kw):
            with pytest.raises(_lib.SFXError) as ei:
                loop.test_phase(kw.pop("W", W), **kw)
            assert f"(status {code})" in str(ei.value) and word in str(ei.value), str(ei.value)

        def valid():
            W.copy_(initial_W(E, d, d, 7))
            _, _, steps = loop.test_phase(W, horizon=4)
            assert steps.tolist() == [4] * E

        refused(-1, "1 <= E <= 64", W=torch.zeros(0, d, device=eng.device))
        valid()
        refused(-1, "1 <= E <= 64", W=torch.zeros(65, d, device=eng.device))
        valid()
        refused(-1, "horizon >= 1", horizon=0)
        valid()
        refused(-1, "w_stride >= d", W=torch.zeros(E, d - 1, device=eng.device))
        valid()
        eng.tsf_setup(8)
        loop.set_schedule("tsf")
        refused(-3, "tsf")
        loop.set_schedule("active")
        valid()
        pre = PreEngine(N_S, d, T, device=eng.device)
        try:
            loop.set_featurizer(pre)
            refused(-3, "featurizer")
            loop.set_featurizer(None)
            valid()
        finally:
            pre.close()
    finally:
        loop.close()
        eng.close()
