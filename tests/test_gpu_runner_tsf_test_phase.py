"""The native runner's TSF test phase (sfx_runner_tsf_test_phase, NativeEnvLoop.tsf_test_phase): E test episodes of
agents/tsfdqn_sequential.py:392-433 stepped in lockstep inside the runner, each row with its own (w, ω), Adam
moments and ω-lr schedule.

  1. bit for bit against a Python loop over SFEngine.tsf_test_actions / tsf_test_updates on the live rows;
  2. against the CPU oracle (oracle.ref_cpu tsf_test_action / tsf_test_update, lr_ω from torch's LambdaLR);
  3. rows whose env reports done get that step's a1 and update and stop;
  4. the optimizer state persists across phases and a non-zero opt_steps start is honoured;
  5. training under schedule "tsf" (look-ahead on) is untouched by a phase;
  6. a second identical phase captures no graph; built-in tasks and schedule are seed-deterministic;
  7. refusals name the limit and leave the runner usable.
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
MAX_BATCH = 16
# non-default hyperparameters, every decay and weight decay non-zero
HP = dict(gamma=0.85, beta=0.5, lasso=0.05, lr_w=2e-3, wd_w=1e-3, lr_omega=5e-3, wd_omega=1e-4, lr_omega_decay=0.01)


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


def problem(T, d, G, K, seed=0):
    """ψ heads as the reference initialises them, target heads a little off the online ones (so ψ⁻ is not ψ),
    random g_t (K planar layers) and h."""
    from sfx.init import reference_heads

    spec = R.Spec(N_S, H, A, d, ("relu", "relu"))
    gs = R.GSpec(N_S, G, K)
    online, w = reference_heads(T, N_S, H, A, d, spec.acts, seed=seed)
    gen = torch.Generator().manual_seed(seed + 7)
    target = online + torch.randn(online.shape, generator=gen) * 1e-2
    g = torch.empty(T, gs.P).uniform_(-0.3, 0.3, generator=gen)
    h = torch.empty(d * G + d).uniform_(-0.1, 0.1, generator=gen)
    return R.TSFState(spec, online.clone(), target.clone(), w.clone(), gspec=gs, g=g, h=h)


def make_engine(st, load_tsf=True):
    from sfx.engine import SFEngine

    spec, gs = st.spec, st.gspec
    eng = SFEngine(st.T, N_S, H, A, spec.d, spec.acts, max_batch=MAX_BATCH)
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    eng.set_target_update_ev(7)
    for t in range(st.T):
        eng.load_head(t, st.online[t], 0)
        eng.load_head(t, st.target[t], 1)
        eng.load_w(t, st.w[t])
    if load_tsf:
        eng.tsf_setup(gs.G, gs.K, 1.0, 1e-3, 0.0, 1e-3, 0.0)
        for t in range(st.T):
            eng.tsf_load_g(t, st.g[t])
        eng.tsf_load_h(st.h)
    return eng


def initial_state(E, T, d, strides, seed):
    """(W, Omega, adam_state) on the CPU at the given row strides: W uniform(-1, 1), ω uniform and normalised,
    zero moments; the columns past d / T / 2(d + T) hold a marker the phase must leave alone."""
    ws, os_, ms = strides
    g = torch.Generator().manual_seed(1000 + seed)
    W = torch.full((E, ws), 7.0)
    W[:, :d] = torch.empty(E, d).uniform_(-1.0, 1.0, generator=g)
    Om = torch.full((E, os_), 7.0)
    om = torch.rand(E, T, generator=g) + 0.05
    Om[:, :T] = om / om.sum(dim=1, keepdim=True)
    M = torch.full((E, ms), 7.0)
    M[:, :2 * (d + T)] = 0.0
    return W, Om, M


def schedule(E, horizon, eps, seed):
    g = np.random.default_rng(500 + seed)
    u = g.random((E, horizon, 2))
    x = g.integers(0, A, (E, horizon, 2))
    return np.where(u <= eps, x, -1).astype(np.int32)


def lr_omega(k):
    from sfx import _lib

    return float(_lib.lib.sfx_tsf_test_lr_omega(HP["lr_omega"], HP["lr_omega_decay"], int(k)))


def python_phase(eng, env, W, Om, M, opt, T, d, explore, horizon):
    """The phase as a Python loop over the existing calls, on the live rows only (compacted as
    sfx.lockstep's TSF kind does): tsf_test_actions(S), the env, tsf_test_actions(S1) with the explored entries
    overwritten, tsf_test_updates with rowp from sfx_tsf_test_lr_omega.  W / Om / M (device, strided) and opt are
    updated in place."""
    E, dev = W.shape[0], eng.device
    nm = 2 * (d + T)
    S = np.stack([env.reset(e) for e in range(E)])
    live = list(range(E))
    ret, loss = np.zeros(E), np.zeros((E, 3))
    steps = np.zeros(E, np.int64)
    acts = np.full((E, horizon, 2), -1, np.int64)
    for j in range(horizon):
        rows = torch.tensor(live, device=dev)
        Wl, Oml, Ml = W[rows, :d].contiguous(), Om[rows, :T].contiguous(), M[rows, :nm].contiguous()
        greedy = eng.tsf_test_actions(torch.from_numpy(S[live]).to(dev), Wl, Oml).cpu().numpy()
        n = len(live)
        S1, PHI = np.zeros((n, N_S), np.float32), np.zeros((n, d), np.float32)
        a_t, rowp, ended = np.zeros(n, np.int64), np.zeros((n, 6), np.float32), []
        for k, e in enumerate(live):
            a = int(explore[e, j, 0]) if explore[e, j, 0] >= 0 else int(greedy[k])
            s1, phi, rr, done = env.step(e, a)
            S1[k], PHI[k], a_t[k] = s1, phi, a
            rowp[k] = [np.float32(rr), HP["lr_w"], HP["wd_w"], lr_omega(opt[e]), HP["wd_omega"], opt[e] + 1]
            opt[e] += 1
            ret[e] += float(np.float32(rr))
            steps[e] += 1
            if done:
                ended.append(e)
        A1 = eng.tsf_test_actions(torch.from_numpy(S1).to(dev), Wl, Oml)
        for k, e in enumerate(live):
            if explore[e, j, 1] >= 0:
                A1[k] = int(explore[e, j, 1])
        lo = eng.tsf_test_updates(torch.from_numpy(S[live]).to(dev), torch.from_numpy(S1).to(dev),
                                  torch.from_numpy(a_t).to(dev), A1, torch.from_numpy(PHI).to(dev), Wl, Oml, Ml,
                                  torch.from_numpy(rowp).to(dev), HP["gamma"], HP["beta"], HP["lasso"]).cpu().numpy()
        W[rows, :d], Om[rows, :T], M[rows, :nm] = Wl, Oml, Ml
        a1 = A1.cpu().numpy()
        for k, e in enumerate(live):
            S[e] = S1[k]
            acts[e, j] = (a_t[k], a1[k])
            loss[e] += lo[k].astype(np.float64)
        live = [e for e in live if e not in ended]
        if not live:
            break
    return ret, loss, steps, acts


def new_loop(eng, seed=3, horizon=HORIZON, **kw):
    from sfx.runner import NativeEnvLoop

    return NativeEnvLoop(eng, batch=16, capacity=100, episode_len=horizon, seed=seed, schedule="tsf", **kw)


def native_phase(eng, E, T, d, strides, seed, done_at=None, horizon=HORIZON, eps=0.3, opt0=0, phases=1):
    """`phases` phases in a row on the same tensors; returns the last phase's outputs and the final state."""
    loop = new_loop(eng, horizon=horizon)
    try:
        W, Om, M = (t.to(eng.device) for t in initial_state(E, T, d, strides, seed))
        opt = np.full(E, opt0, np.int64)
        for p in range(phases):
            loop.set_test_env(DetEnv(E, d, seed + 100 * p, done_at))
            ret, loss, steps, acts = loop.tsf_test_phase(W, Om, M, opt, HP, explore=schedule(E, horizon, eps, seed + p),
                                                         want_actions=True)
        return dict(ret=ret.copy(), loss=loss.copy(), steps=steps.copy(), acts=acts.copy(), W=W.cpu(), Om=Om.cpu(),
                    M=M.cpu(), opt=opt.copy())
    finally:
        loop.close()


def python_phases(eng, E, T, d, strides, seed, done_at=None, horizon=HORIZON, eps=0.3, opt0=0, phases=1):
    W, Om, M = (t.to(eng.device) for t in initial_state(E, T, d, strides, seed))
    opt = np.full(E, opt0, np.int64)
    for p in range(phases):
        ret, loss, steps, acts = python_phase(eng, DetEnv(E, d, seed + 100 * p, done_at), W, Om, M, opt, T, d,
                                              schedule(E, horizon, eps, seed + p), horizon)
    return dict(ret=ret, loss=loss, steps=steps, acts=acts, W=W.cpu(), Om=Om.cpu(), M=M.cpu(), opt=opt)


def same(got, ref, rows=None):
    rows = range(len(got["steps"])) if rows is None else rows
    for e in rows:
        assert np.array_equal(got["acts"][e], ref["acts"][e]), (e, got["acts"][e], ref["acts"][e])
        for k in ("W", "Om", "M"):
            assert torch.equal(got[k][e], ref[k][e]), (e, k)
        assert got["opt"][e] == ref["opt"][e] and got["steps"][e] == ref["steps"][e]
        assert got["ret"][e] == ref["ret"][e]
        assert got["loss"][e].tolist() == ref["loss"][e].tolist()


BASE = (5, 4, 8, 8, 0, (8, 4, 24))


@pytest.fixture(scope="module")
def base():
    """The phase of BASE without early ends, computed once (tests 1 and 3)."""
    if not gpu_available():
        pytest.skip("no HIP device")
    E, T, d, G, K, strides = BASE
    eng = make_engine(problem(T, d, G, K))
    try:
        return native_phase(eng, E, T, d, strides, seed=1)
    finally:
        eng.close()


@pytest.mark.parametrize("E,T,d,G,K,strides", [BASE, (13, 3, 20, 12, 3, (24, 8, 64)), (16, 6, 12, 12, 0, (12, 6, 36)),
                                               (1, 1, 8, 8, 0, (8, 1, 18))])
def test_phase_bit_for_bit_against_existing_calls(E, T, d, G, K, strides, base):
    """A ragged tile; planar flows and every stride wider than its row; E = max_batch; a single row and head."""
    seed = 2 if E == 1 else 1  # the single row's 9 steps explore in both columns under seed 2
    ex = schedule(E, HORIZON, 0.3, seed)
    for c in (0, 1):  # explored and greedy entries in both columns
        assert (ex[:, :, c] >= 0).any() and (ex[:, :, c] < 0).any()
    eng = make_engine(problem(T, d, G, K))
    try:
        got = base if (E, T, d, G, K, strides) == BASE else native_phase(eng, E, T, d, strides, seed=seed)
        ref = python_phases(eng, E, T, d, strides, seed=seed)
    finally:
        eng.close()
    assert (got["acts"] >= 0).all() and (got["acts"] < A).all()
    same(got, ref)
    assert got["steps"].tolist() == [HORIZON] * E and got["opt"].tolist() == [HORIZON] * E
    W0, Om0, M0 = initial_state(E, T, d, strides, seed)
    assert not torch.equal(got["W"][:, :d], W0[:, :d]) and not torch.equal(got["Om"][:, :T], Om0[:, :T])
    # the columns past a row's own are the caller's
    assert torch.equal(got["W"][:, d:], W0[:, d:]) and torch.equal(got["Om"][:, T:], Om0[:, T:])
    assert torch.equal(got["M"][:, 2 * (d + T):], M0[:, 2 * (d + T):])


def oracle_phase(st, env, W, Om, explore, horizon):
    """The phase on the CPU oracle, lr_ω from torch's own LambdaLR.  Returns (actions, loss sums, final W, final
    Ω, the smallest top-2 gap of a greedy choice relative to the largest |q|)."""
    E, T = W.shape[0], st.T
    acts = np.full((E, horizon, 2), -1, np.int64)
    loss = np.zeros((E, 3))
    min_gap = float("inf")

    def choose(s, tm, x):
        nonlocal min_gap
        if x >= 0:
            return int(x)
        on = tm.omega / tm.omega.sum()
        psi = R.psi_all(st.online, st.spec, s.reshape(1, -1))[0]
        q = (psi * on.view(-1, 1, 1)).sum(0) @ tm.w
        top = torch.topk(q, 2).values
        min_gap = min(min_gap, float(top[0] - top[1]) / float(q.abs().max()))
        return R.tsf_test_action(st, s, tm.w, tm.omega)

    for e in range(E):
        tm = R.TestMapper(W[e].clone(), Om[e].clone())
        p = torch.nn.Parameter(torch.zeros(1))
        optim = torch.optim.Adam([{"params": [p], "lr": HP["lr_omega"]}])
        sched = torch.optim.lr_scheduler.LambdaLR(optim, lambda epoch: (1 - HP["lr_omega_decay"]) ** epoch)
        s = torch.from_numpy(env.reset(e))
        for j in range(horizon):
            a = choose(s, tm, explore[e, j, 0])
            s1, phi, r, _ = env.step(e, a)
            s1 = torch.from_numpy(s1)
            a1 = choose(s1, tm, explore[e, j, 1])
            lo = R.tsf_test_update(st, tm, s, a, float(np.float32(r)), torch.from_numpy(phi), s1, a1, gamma=HP["gamma"],
                                   beta=HP["beta"], lasso=HP["lasso"], lr_w=HP["lr_w"], wd_w=HP["wd_w"],
                                   lr_o=optim.param_groups[0]["lr"], wd_o=HP["wd_omega"])
            optim.step()
            sched.step()
            loss[e] += lo
            acts[e, j] = (a, a1)
            s = s1
        W[e], Om[e] = tm.w, tm.omega
    return acts, loss, min_gap


def oracle_case(seed):
    E, T, d, G, K = 5, 4, 8, 8, 3
    st = problem(T, d, G, K)
    W, Om, _ = initial_state(E, T, d, (d, T, 2 * (d + T)), seed)
    acts, loss, gap = oracle_phase(st, DetEnv(E, d, seed), W, Om, schedule(E, HORIZON, 0.3, seed), HORIZON)
    return st, acts, loss, W, Om, gap


def test_phase_against_oracle():
    E, T, d = 5, 4, 8
    # the seed is picked on the CPU from the oracle alone: the first whose greedy choices are no near ties
    for seed in range(256):
        st, acts, loss, W_ref, Om_ref, gap = oracle_case(seed)
        if gap > 1e-3:
            break
    assert gap > 1e-3, gap
    eng = make_engine(st)
    try:
        got = native_phase(eng, E, T, d, (d, T, 2 * (d + T)), seed=seed)
    finally:
        eng.close()
    assert np.array_equal(got["acts"], acts)  # every step, none excluded
    rel_close(got["W"], W_ref, rtol=1e-4, atol=1e-7)
    rel_close(got["Om"], Om_ref, rtol=1e-4, atol=1e-7)
    rel_close(got["loss"], loss, rtol=1e-4, atol=1e-7)
    assert got["steps"].tolist() == [HORIZON] * E


def test_phase_early_end(base):
    E, T, d, G, K, strides = BASE
    done_at = {2: 3, 0: HORIZON - 1, 4: 0}
    eng = make_engine(problem(T, d, G, K))
    try:
        got = native_phase(eng, E, T, d, strides, seed=1, done_at=done_at)
        ref = python_phases(eng, E, T, d, strides, seed=1, done_at=done_at)
        # every row ends by step 2: the call returns, no wait runs out
        early = native_phase(eng, E, T, d, strides, seed=1, done_at={0: 2, 1: 0, 2: 1, 3: 2, 4: 0})
    finally:
        eng.close()
    assert got["steps"].tolist() == [HORIZON, HORIZON, 4, HORIZON, 1] and ref["steps"].tolist() == got["steps"].tolist()
    assert got["opt"].tolist() == got["steps"].tolist()
    same(got, ref, rows=(2, 4))  # the Python loop's rows after 4 and 1 updates
    for e, n in ((2, 4), (4, 1)):
        assert (got["acts"][e, n:] == -1).all() and (got["acts"][e, :n] >= 0).all()
        assert not torch.equal(got["W"][e], base["W"][e]) and not torch.equal(got["M"][e], base["M"][e])
    same(got, base, rows=(0, 1, 3))  # row 0 ends at the last step: nothing of it changes
    assert early["steps"].tolist() == [3, 1, 2, 3, 1] and (early["steps"] <= 3).all()
    assert early["opt"].tolist() == early["steps"].tolist()
    for e in range(E):
        n = early["steps"][e]
        assert (early["acts"][e, n:] == -1).all() and (early["acts"][e, :n] >= 0).all()


def test_optimizer_state_across_phases():
    E, T, d, G, K, strides = BASE
    eng = make_engine(problem(T, d, G, K))
    try:
        got = native_phase(eng, E, T, d, strides, seed=2, phases=2)
        ref = python_phases(eng, E, T, d, strides, seed=2, phases=2)
        got37 = native_phase(eng, E, T, d, strides, seed=2, opt0=37)
        ref37 = python_phases(eng, E, T, d, strides, seed=2, opt0=37)
        got0 = native_phase(eng, E, T, d, strides, seed=2)
    finally:
        eng.close()
    same(got, ref)
    assert got["opt"].tolist() == [2 * HORIZON] * E
    same(got37, ref37)
    assert got37["opt"].tolist() == [37 + HORIZON] * E
    assert not torch.equal(got37["W"], got0["W"])  # the step number and ω's lr did reach the update


def _training_state(eng, loop, T):
    heads = [torch.stack([eng.get_head(t, which) for t in range(T)]) for which in (0, 1)]
    adam = [eng.get_adam(t) for t in range(T)]
    w = [eng.get_w(t) for t in range(T)]
    g = [eng.tsf_get_g(t) for t in range(T)]
    hs = [eng.tsf_get_h_state(t) for t in range(T)]
    return {"heads": heads, "m": torch.stack([a[0] for a in adam]), "v": torch.stack([a[1] for a in adam]),
            "steps": [a[2] for a in adam], "w": torch.stack([torch.cat([x.reshape(-1) for x in ww]) for ww in w]),
            "since": [eng.since_target(t) for t in range(T)], "gpi": loop.gpi_counters(),
            "g": torch.stack([torch.cat(x) for x in g]), "h": eng.tsf_get_h(),
            "hs": torch.stack([torch.cat(x) for x in hs])}


def test_training_untouched_by_a_phase():
    """Schedule tsf with the default switches (look-ahead on): two runs, with and without a phase between."""
    from sfx.runner import NativeEnvLoop

    T, d, G, K, E = 3, 8, 8, 2, 5

    def run(with_phase):
        st = problem(T, d, G, K)
        eng = make_engine(st)
        loop = NativeEnvLoop(eng, batch=16, capacity=200, gamma=0.9, epsilon=0.3, episode_len=7, seed=5, schedule="tsf")
        try:
            loop.prefill(20)
            loop.set_task(0)
            loop.run(30)
            if with_phase:
                W, Om, M = (t.to(eng.device) for t in initial_state(E, T, d, (d, T, 2 * (d + T)), 2))
                opt = np.zeros(E, np.int64)
                _, _, steps = loop.tsf_test_phase(W, Om, M, opt, HP, horizon=HORIZON, test_epsilon=0.3)
                assert steps.tolist() == [HORIZON] * E
            loop.record(40)
            loop.run(30)
            loop.set_task(1)
            loop.run(10)
            recs = loop.records()
            assert len(recs) == 40
            s = _training_state(eng, loop, T)
            s["actions"] = [(r["task"], r["c"], r["a_greedy"], r["a_taken"]) for r in recs]
            s["stats"] = loop.stats()
            return s, st
        finally:
            loop.close()
            eng.close()

    (a, st), (b, _) = run(True), run(False)
    for x, y in zip(a["heads"], b["heads"]):
        assert torch.equal(x, y)
    for k in ("m", "v", "w", "g", "h", "hs"):
        assert torch.equal(a[k], b[k]), k
    assert a["steps"] == b["steps"] and a["since"] == b["since"] and np.array_equal(a["gpi"], b["gpi"])
    assert a["actions"] == b["actions"]
    assert a["stats"]["ahead_pre_steps"] == b["stats"]["ahead_pre_steps"]
    assert sum(a["steps"]) > 0 and not torch.equal(a["h"], st.h)  # the runs did train


def test_graph_reuse_and_determinism():
    E, T, d, G, K, strides = BASE

    def builtin(seed, phases=1):
        eng = make_engine(problem(T, d, G, K))
        loop = new_loop(eng, seed=seed)
        try:
            caps = []
            for _ in range(phases):
                if not caps:
                    W, Om, M = (t.to(eng.device) for t in initial_state(E, T, d, strides, 6))
                else:
                    for t, t0 in zip((W, Om, M), initial_state(E, T, d, strides, 6)):
                        t.copy_(t0)
                opt = np.zeros(E, np.int64)
                ret, loss, steps, acts = loop.tsf_test_phase(W, Om, M, opt, HP, test_epsilon=0.3, want_actions=True)
                caps.append(eng.graph_stats()["captures"])
            return ret.copy(), acts.copy(), W.cpu(), Om.cpu(), caps
        finally:
            loop.close()
            eng.close()

    # two phases with the same arguments: the second captures nothing (at most two graphs in the first)
    *_, caps = builtin(21, phases=2)
    assert caps[1] == caps[0] and 1 <= caps[0] <= 2
    r1, a1, w1, o1, _ = builtin(21)
    r2, a2, w2, o2, _ = builtin(21)
    assert r1.tolist() == r2.tolist() and np.array_equal(a1, a2) and torch.equal(w1, w2) and torch.equal(o1, o2)
    r3, a3, _, _, _ = builtin(22)
    assert not np.array_equal(a1, a3) and r1.tolist() != r3.tolist()
    assert (a1 >= 0).all() and (a1 < A).all()


def test_refusals_leave_the_runner_usable():
    from sfx import _lib

    E, T, d, G, K, strides = BASE
    st = problem(T, d, G, K)
    eng = make_engine(st)
    bare = make_engine(st, load_tsf=False)
    loop = new_loop(eng, seed=2)
    try:
        dev = eng.device
        state = [t.to(dev) for t in initial_state(E, T, d, strides, 7)]

        def refused(code, word, on=loop, opt=None, **kw):
            t = [kw.pop(k, state[i]) for i, k in enumerate(("W", "Om", "M"))]
            opt = np.zeros(t[0].shape[0], np.int64) if opt is None else opt
            with pytest.raises(_lib.SFXError) as ei:
                on.tsf_test_phase(t[0], t[1], t[2], opt, HP, **kw)
            assert f"(status {code})" in str(ei.value) and word in str(ei.value), str(ei.value)

        def valid():
            for t, t0 in zip(state, initial_state(E, T, d, strides, 7)):
                t.copy_(t0)
            opt = np.zeros(E, np.int64)
            _, _, steps = loop.tsf_test_phase(*state, opt, HP, horizon=4)
            assert steps.tolist() == [4] * E and opt.tolist() == [4] * E
            loop.run(5)

        def zeros(n, strides_=strides):
            return dict(zip(("W", "Om", "M"), (torch.zeros(n, s, device=dev) for s in strides_)))

        loop.set_schedule("all")
        refused(-3, "tsf schedule only")
        loop.set_schedule("tsf")
        loop.prefill(20)
        loop.set_task(0)
        valid()
        refused(-1, "1 <= E <= min(64, max_batch = 16)", **zeros(0))
        valid()
        refused(-1, "1 <= E <= min(64, max_batch = 16)", **zeros(MAX_BATCH + 1))
        valid()
        refused(-1, "o_stride >= T", Om=torch.zeros(E, T - 1, device=dev))
        valid()
        refused(-1, "mom_stride >= 2(d + T)", M=torch.zeros(E, 2 * (d + T) - 1, device=dev))
        valid()
        bad = np.full((E, HORIZON, 2), -1, np.int32)
        bad[3, 2, 1] = A
        refused(-1, "action >= A", explore=bad)
        valid()
        refused(-1, "opt_steps >= 0", opt=np.array([0, 0, -1, 0, 0], np.int64))
        valid()
        other = NativeEnvLoop_all(bare)
        try:
            other.prefill(20)
            other.set_task(0)
            refused(-3, "sfx_tsf_setup", on=other)
            other.run(5)
        finally:
            other.close()
        valid()
    finally:
        loop.close()
        eng.close()
        bare.close()


def NativeEnvLoop_all(eng):
    from sfx.runner import NativeEnvLoop

    return NativeEnvLoop(eng, batch=16, capacity=100, episode_len=HORIZON, seed=2, schedule="all")
