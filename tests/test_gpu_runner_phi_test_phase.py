"""The native runner's test phase of the learned-φ SF agent (sfx_runner_phi_test_phase, NativeEnvLoop.phi_test_phase
and .train under schedule "phi"; k_phi_test_intake / k_phi_test_row in csrc/sfx_testphase.h): E test episodes of
agents/sfdqn_phi.py:234-261 stepped in lockstep inside the runner.

  1. bit for bit against a Python loop of SFEngine.phi_test_actions + SFEngine.phi_test_updates on the live rows;
  2. against the CPU restatement (tests/phi_test_ref.py sf_greedy / sf_update in float32 torch);
  3. a tie made by the bias goes to the first index, through the phase;
  4. training under "phi" is untouched by a phase (heads, φ net, Adam state, w, bias and λ scalars, target and GPI
     counters, phi_losses, the next 40 recorded steps);
  5. a second identical phase captures no graph; built-in tasks and the drawn schedule are seed-deterministic;
  6. refusals name the limit and leave the runner usable.

Shapes (tests/test_gpu_phi_runner.py's, the smallest that reach every φ kernel family): ψ Spec(11, 32, 5, 6) --
n_in = 23 odd, d = 6 no multiple of 4 -- T = 3, max_batch 16; φ nets narrow (k_phiE_narrow), w132 (16-byte rows
through LDS: two launches at E = 9) and w131 (scalar-load rows: the <16> accumulators at E = 9); horizon 9.

Bounds of test 2 are tests/test_gpu_phi_lockstep.py's for one update (rtol 1e-5, a floor of one fp32 ulp of the
largest pre-step parameter).  They hold over a phase because a freshly built Adam's first step is
lr · g / (|g| + eps): a parameter moves by lr to within eps / |g| whatever the last bits of g are, so a step's
rounding does not grow over the steps; the env's rewards keep |ρ| above 1, far from a gradient of rounding size.
"""
import numpy as np
import pytest
import torch

from tests import phi_test_ref as PT
from tests.conftest import gpu_available
from tests.test_gpu_phi_runner import EV, NETS, SPEC, T_, make_state
from tests.test_gpu_tsf_phi import engine_of, gpu_state

pytestmark = pytest.mark.gpu

N_S, A, D = SPEC.n_s, SPEC.A, SPEC.d
HORIZON = 9
MAXB = 16
ORACLE_SEED = 1  # test 2's env / W / schedule seed: its top-2 gap precondition holds (asserted there)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


class DetEnv:
    """Deterministic test tasks: task e's stream depends only on (seed, e) and the actions it was given.  No φ: the
    phase computes it from (s, a, s1).  r stays in [3, 4): |w·φ + b - r| > 1 for the reward models used here.
    done_at: {e: step index at which task e reports done}."""

    def __init__(self, E, seed, done_at=None):
        self.E, self.seed, self.done_at = E, seed, dict(done_at or {})
        self.rng = [None] * E
        self.t = [0] * E

    def reset(self, e):
        self.rng[e] = np.random.default_rng([self.seed, e])
        self.t[e] = 0
        return self.rng[e].standard_normal(N_S, dtype=np.float32)

    def step(self, e, a):
        g = self.rng[e]
        s1 = g.standard_normal(N_S, dtype=np.float32) + np.float32(0.05 * a)
        r = np.float32(3.0) + np.float32(0.5) * g.random(dtype=np.float32) + np.float32(0.125) * np.float32(a % 3)
        done = self.done_at.get(e) == self.t[e]
        self.t[e] += 1
        return s1, None, float(r), done


def make_engine(st, net):
    return engine_of(st, EV, max_batch=MAXB, tsf=False, phi=NETS[net][2])


def make_loop(eng, schedule="phi", **kw):
    from sfx.runner import NativeEnvLoop

    args = dict(batch=16, capacity=200, gamma=0.9, epsilon=0.3, episode_len=HORIZON, seed=9, schedule=schedule,
                p_end=0.1 if schedule == "phi" else 0.0, phi_bias=eng.test_wb, phi_lambda=eng.test_lam)
    args.update(kw)
    return NativeEnvLoop(eng, **args)


def initial_W(E, stride, seed):
    """(W [E, stride], Wb [E]); the columns past d hold 7: the phase must leave them alone."""
    g = torch.Generator().manual_seed(1000 + seed)
    W = torch.full((E, stride), 7.0)
    W[:, :D] = torch.empty(E, D).uniform_(-0.5, 0.5, generator=g)
    return W, torch.empty(E).uniform_(-0.4, 0.4, generator=g)


def schedule(E, horizon, eps, seed):
    g = np.random.default_rng(500 + seed)
    u = g.random((E, horizon))
    x = g.integers(0, A, (E, horizon))
    return np.where(u <= eps, x, -1).astype(np.int32)


def python_phase(eng, env, W, Wb, explore, horizon):
    """The phase as a Python loop over the existing calls, as sfx.lockstep's SF-φ kind makes them: per lockstep
    step one phi_test_actions and one phi_test_updates on the rows that still run (gathered, then scattered)."""
    E, dev = W.shape[0], eng.device
    S = np.stack([env.reset(e) for e in range(E)])
    live = list(range(E))
    ret, loss = np.zeros(E), np.zeros(E)
    steps = np.zeros(E, np.int64)
    acts = np.full((E, horizon), -1, np.int64)
    for j in range(horizon):
        rows = torch.tensor(live, device=dev)
        Wl, Wbl = W[rows, :D].contiguous(), Wb[rows].contiguous()
        Sl = torch.from_numpy(S[live]).to(dev)
        sel = eng.phi_test_actions(Sl, Wl, Wbl).cpu().numpy()
        a_l, r_l, s1_l, ended = [], [], [], []
        for k, e in enumerate(live):
            a = int(explore[e, j]) if explore[e, j] >= 0 else int(sel[k, 1])
            s1, _, r, done = env.step(e, a)
            a_l.append(a)
            r_l.append(np.float32(r))
            s1_l.append(s1)
            acts[e, j] = a
            ret[e] += float(np.float32(r))
            steps[e] += 1
            if done:
                ended.append(e)
        lo = eng.phi_test_updates(Sl, torch.tensor(a_l, dtype=torch.long), torch.tensor(np.array(r_l)),
                                  torch.from_numpy(np.stack(s1_l)), Wl, Wbl).cpu()
        W[rows, :D] = Wl
        Wb[rows] = Wbl
        for k, e in enumerate(live):
            loss[e] += float(lo[k])
            S[e] = s1_l[k]
        live = [e for e in live if e not in ended]
        if not live:
            break
    return ret, loss, steps, acts


def native_phases(eng, E, stride, seed, done_at=None, horizon=HORIZON, eps=0.3, phases=1):
    """`phases` consecutive phases on the same (W, Wb): [(ret, loss, steps, acts, W, Wb) after each]."""
    loop = make_loop(eng)
    try:
        W, Wb = (t.to(eng.device) for t in initial_W(E, stride, seed))
        out = []
        for p in range(phases):
            loop.set_test_env(DetEnv(E, seed + p, done_at))
            ret, loss, steps, acts = loop.phi_test_phase(W, Wb, explore=schedule(E, horizon, eps, seed + p),
                                                         want_actions=True)
            out.append((ret.copy(), loss.copy(), steps.copy(), acts.copy(), W.cpu(), Wb.cpu()))
        return out
    finally:
        loop.close()


# ---- 1. bit for bit against the existing calls ----------------------------------------------------
# (net, E, w_stride, rows that end: {row: step}).  E = 9: w132 takes two LDS launches, w131 the <16> accumulators;
# E = 16 = max_batch; rows end at step 0, in the middle and at the last step
CASES = [("narrow", 1, D, None), ("narrow", 3, D + 3, {1: 0}), ("narrow", 9, D, {0: 4, 8: HORIZON - 1}),
         ("narrow", 16, D + 3, {15: 0, 3: 5}),
         ("w132", 1, D + 3, {0: 4}), ("w132", 3, D, None), ("w132", 9, D + 3, {8: 0, 2: 3, 5: HORIZON - 1}),
         ("w132", 16, D, {7: 2}),
         ("w131", 1, D, None), ("w131", 3, D + 3, {0: HORIZON - 1, 2: 0}), ("w131", 9, D, {4: 4}),
         ("w131", 16, D + 3, {0: 0, 9: 6, 15: HORIZON - 1})]


@pytest.mark.parametrize("net,E,stride,done_at", CASES)
def test_phase_bit_for_bit_against_existing_calls(net, E, stride, done_at):
    st = make_state(net)
    eng = make_engine(st, net)
    try:
        got = native_phases(eng, E, stride, seed=1, done_at=done_at, phases=2)
        W, Wb = (t.to(eng.device) for t in initial_W(E, stride, 1))
        for p in range(2):
            explore = schedule(E, HORIZON, 0.3, 1 + p)
            ret, loss, steps, acts = python_phase(eng, DetEnv(E, 1 + p, done_at), W, Wb, explore, HORIZON)
            g = got[p]
            want_steps = [(done_at or {}).get(e, HORIZON - 1) + 1 for e in range(E)]
            assert g[2].tolist() == want_steps and steps.tolist() == want_steps
            assert np.array_equal(g[3], acts), (p, g[3], acts)
            for e in range(E):
                assert (g[3][e, :want_steps[e]] >= 0).all() and (g[3][e, want_steps[e]:] == -1).all()
            assert torch.equal(g[4], W.cpu()) and torch.equal(g[5], Wb.cpu()), p
            assert g[1].tolist() == loss.tolist()
            assert g[0].tolist() == ret.tolist()
            if E * HORIZON >= 27:  # both kinds of step occur
                assert (explore >= 0).any() and (explore < 0).any()
        w0, wb0 = initial_W(E, stride, 1)
        assert torch.equal(got[1][4][:, D:], w0[:, D:])  # the padding columns
        assert not torch.equal(got[0][4][:, :D], w0[:, :D]) and not torch.equal(got[0][5], wb0)
        assert not torch.equal(got[1][4], got[0][4])  # the second phase went on from the first one's rows
        assert torch.equal(eng.phi_get(), st.phi)
    finally:
        eng.close()


# ---- 2. against the CPU restatement -----------------------------------------------------------------
def reference_phase(st, env, W, Wb, explore, horizon):
    """The phase in float32 torch on the CPU: SFDQN_PHI.get_test_action's greedy branch (PT.sf_greedy: GPI_w with
    the biased Linear) and update_test_reward_mapper (PT.sf_update).  W [E, d], Wb [E] in place.  Returns
    (actions, loss sums, the smallest top-2 gap of q over the phase's greedy steps divided by the largest |q| of the
    whole phase, the largest pre-step |parameter|)."""
    E = W.shape[0]
    S = [torch.from_numpy(env.reset(e)) for e in range(E)]
    acts = np.full((E, horizon), -1, np.int64)
    loss = np.zeros(E)
    min_gap, q_max, pmax = float("inf"), 0.0, 0.0
    for j in range(horizon):
        for e in range(E):
            tt = PT.TestTask(torch.zeros(1), torch.zeros(1), W[e], Wb[e:e + 1], torch.ones(1))
            a, gap, qmax = PT.sf_greedy(st, tt, S[e])
            q_max = max(q_max, qmax)
            if explore[e, j] >= 0:
                a = int(explore[e, j])
            else:
                min_gap = min(min_gap, gap)
            s1, _, r, _ = env.step(e, a)
            s1 = torch.from_numpy(s1)
            pmax = max(pmax, float(W[e].abs().max()), float(Wb[e].abs()))
            loss[e] += PT.sf_update(st, tt, S[e], a, float(np.float32(r)), s1)  # tt.w / tt.wb are views of W / Wb
            S[e] = s1
            acts[e, j] = a
    return acts, loss, min_gap / q_max, pmax


def oracle_case(net, seed):
    E = 5
    st = make_state(net)
    W, Wb = initial_W(E, D, seed)
    acts, loss, min_gap, pmax = reference_phase(st, DetEnv(E, seed), W, Wb, schedule(E, HORIZON, 0.3, seed), HORIZON)
    return st, W, Wb, acts, loss, min_gap, pmax


@pytest.mark.parametrize("net", ["narrow", "w132"])
def test_phase_against_the_cpu_restatement(net):
    E = 5
    st, W_ref, Wb_ref, acts, loss, min_gap, pmax = oracle_case(net, ORACLE_SEED)
    # the test's own precondition, on the reference alone: no greedy step of it is a near tie
    assert min_gap > 1e-3, min_gap
    eng = make_engine(st, net)
    try:
        ret, lsum, steps, got_acts, W, Wb = native_phases(eng, E, D, seed=ORACLE_SEED)[0]
    finally:
        eng.close()
    floor = float(np.spacing(np.float32(pmax)))
    print(f"{net}: min gap {min_gap:.3e}, floor {floor:.3e}, max |W - ref| {float((W - W_ref).abs().max()):.3e}, "
          f"max |Wb - ref| {float((Wb - Wb_ref).abs().max()):.3e}, loss sums {lsum.tolist()} ref {loss.tolist()}")
    assert np.array_equal(got_acts, acts)  # every step, none excluded
    np.testing.assert_allclose(W.numpy(), W_ref.numpy(), rtol=1e-5, atol=floor)
    np.testing.assert_allclose(Wb.numpy(), Wb_ref.numpy(), rtol=1e-5, atol=floor)
    np.testing.assert_allclose(lsum, loss, rtol=1e-5, atol=1e-12)
    assert steps.tolist() == [HORIZON] * E


# ---- 3. the bias makes the tie ------------------------------------------------------------------------
def test_tie_made_by_the_bias_through_the_phase():
    """tests/test_gpu_phi_lockstep.py::test_biased_selection_tie_made_by_the_bias' construction: two q one ulp
    apart, the larger at the later index; a bias of 4 rounds both to 5, so the first index wins while the unbiased
    selection picks the later one.  ψ is pinned through the heads' output layer (zero weights, the values in the
    bias), w = e_0, so every state gives the same q; the phase's first step (horizon 1) takes that action."""
    lo, hi, bias = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)), np.float32(4.0)
    assert hi > lo and np.float32(lo + bias) == np.float32(hi + bias) == np.float32(5.0)
    st = make_state("narrow", seed=61)
    net = st.net
    n_out = net.A * net.d
    for t in range(T_):
        st.online[t, -(n_out * net.H + n_out):] = 0.0
    st.online[0, -n_out + 1 * net.d] = float(lo)   # ψ_0[a = 1][0]
    st.online[1, -n_out + 2 * net.d] = float(hi)   # ψ_1[a = 2][0]
    eng = make_engine(st, "narrow")
    loop = make_loop(eng)
    try:
        E = 3
        W = torch.zeros(E, D, device=eng.device)
        W[:, 0] = 1.0
        Wb = torch.tensor([float(bias), 0.0, float(bias)], device=eng.device)
        loop.set_test_env(DetEnv(E, 3))
        S0 = torch.from_numpy(np.stack([DetEnv(E, 3).reset(e) for e in range(E)])).to(eng.device)
        assert eng.test_actions(S0, W).cpu().tolist() == [[1, 2]] * E  # without a bias: the later, larger one
        assert eng.phi_test_actions(S0, W.clone(), Wb.clone()).cpu().tolist() == [[0, 1], [1, 2], [0, 1]]
        _, _, steps, acts = loop.phi_test_phase(W, Wb, horizon=1, explore=np.full((E, 1), -1, np.int32),
                                                want_actions=True)
        assert steps.tolist() == [1] * E
        assert acts.tolist() == [[1], [2], [1]]  # rows 0 and 2: the tie, the first index; row 1 has no bias
    finally:
        loop.close()
        eng.close()


# ---- 4. training is untouched ---------------------------------------------------------------------------
def _training_state(eng, loop):
    st = gpu_state(eng, T_, tsf=False)  # heads, w, the φ net, the bias and λ scalars
    adam = [eng.get_adam(t) for t in range(T_)]
    st["m"] = torch.stack([a[0] for a in adam])
    st["v"] = torch.stack([a[1] for a in adam])
    other = {"steps": [a[2] for a in adam], "since": [eng.since_target(t) for t in range(T_)],
             "gpi": loop.gpi_counters().tolist(), "phi_losses": loop.phi_losses()}
    return st, other


@pytest.mark.parametrize("net", ["narrow", "w132"])
def test_training_untouched_by_a_phase(net):
    """The phase in the middle uses the built-in test tasks and draws its own schedule (explore=None), so it also
    shows that neither moves a training stream."""
    E = 5

    def run(with_phase):
        st = make_state(net)
        eng = make_engine(st, net)
        loop = make_loop(eng, episode_len=7)
        try:
            loop.prefill(20)
            loop.set_task(2)
            loop.run(30)
            if with_phase:
                W, Wb = (t.to(eng.device) for t in initial_W(E, D, 2))
                _, _, steps = loop.phi_test_phase(W, Wb, horizon=HORIZON, test_epsilon=0.3)
                assert steps.tolist() == [HORIZON] * E
                assert not torch.equal(W.cpu(), initial_W(E, D, 2)[0])
            loop.record(40)
            loop.run(30)
            loop.set_task(1)
            loop.run(10)
            recs = loop.records()
            assert len(recs) == 40
            tensors, other = _training_state(eng, loop)
            other["actions"] = [(r["task"], r["c"], r["a_greedy"], r["a_taken"]) for r in recs]
            return tensors, other
        finally:
            loop.close()
            eng.close()

    (ta, oa), (tb, ob) = run(True), run(False)
    for name in ta:
        assert torch.equal(ta[name], tb[name]), name
    assert oa == ob
    assert not torch.equal(ta["phi"], make_state(net).phi)  # the runs did train


# ---- 5. determinism and caching -------------------------------------------------------------------------
def test_graph_reuse_and_determinism():
    E = 5

    def builtin(seed, phases=1):
        st = make_state("w132")
        eng = make_engine(st, "w132")
        loop = make_loop(eng, seed=seed)
        try:
            W, Wb = (t.to(eng.device) for t in initial_W(E, D, 6))  # the same buffers: the graph is keyed on them
            caps = [eng.graph_stats()["captures"]]
            for _ in range(phases):
                w0, b0 = initial_W(E, D, 6)
                W.copy_(w0)
                Wb.copy_(b0)
                ret, loss, steps, acts = loop.phi_test_phase(W, Wb, test_epsilon=0.3, want_actions=True)
                caps.append(eng.graph_stats()["captures"])
            return ret.copy(), acts.copy(), W.cpu(), Wb.cpu(), caps
        finally:
            loop.close()
            eng.close()

    # two phases with the same arguments: one graph in the first, none in the second
    *_, caps = builtin(21, phases=2)
    assert caps[1] == caps[0] + 1 and caps[2] == caps[1], caps
    r1, a1, w1, b1, _ = builtin(21)
    r2, a2, w2, b2, _ = builtin(21)
    assert r1.tolist() == r2.tolist() and np.array_equal(a1, a2) and torch.equal(w1, w2) and torch.equal(b1, b2)
    r3, a3, *_ = builtin(22)
    assert not np.array_equal(a1, a3) and r1.tolist() != r3.tolist()
    assert (a1 >= 0).all() and (a1 < A).all()


def test_train_evaluates_with_the_phase_under_phi():
    """NativeEnvLoop.train under "phi": n_test_ev = 10 over 25 steps evaluates after steps 1, 11 and 21 of every
    task, moves the reward models and leaves the training state of the same runs without phases."""
    from sfx.runner import test_phase_steps

    E, n = 3, 25
    out = []
    for with_phase in (True, False):
        st = make_state("narrow")
        eng = make_engine(st, "narrow")
        loop = make_loop(eng, episode_len=7)
        try:
            loop.prefill(20)
            if with_phase:
                W, Wb = (t.to(eng.device) for t in initial_W(E, D, 4))
                data = loop.train([0, 2], n, W, n_test_ev=10, Wb=Wb, horizon=6)
                assert len(data) == 3 * 2 and all(isinstance(v, np.float32) and np.isfinite(v) for v in data)
                assert not torch.equal(W.cpu(), initial_W(E, D, 4)[0]) and not torch.equal(Wb.cpu(), initial_W(E, D, 4)[1])
            else:
                for task in (0, 2):
                    loop.set_task(task)
                    done = 0
                    for t in test_phase_steps(n, 10):
                        loop.run(t + 1 - done)
                        done = t + 1
                    loop.run(n - done)
            assert loop.stats()["env_steps"] == 2 * n
            out.append(_training_state(eng, loop))
        finally:
            loop.close()
            eng.close()
    for name in out[0][0]:
        assert torch.equal(out[0][0][name], out[1][0][name]), name
    assert out[0][1] == out[1][1]


# ---- 6. refusals ----------------------------------------------------------------------------------------
def test_refusals_leave_the_runner_usable():
    import ctypes as C

    from sfx import _lib
    from sfx.pretrain import PreEngine

    E = 5
    st = make_state("narrow")
    eng = make_engine(st, "narrow")
    loop = make_loop(eng)
    try:
        dev = eng.device
        W, Wb = (t.to(dev) for t in initial_W(E, D, 7))

        def refused(code, word, **kw):
            with pytest.raises(_lib.SFXError) as ei:
                loop.phi_test_phase(kw.pop("W", W), kw.pop("Wb", Wb), **kw)
            assert f"(status {code})" in str(ei.value) and word in str(ei.value), str(ei.value)

        def raw(code, word, W_ptr, Wb_ptr, explore=None):
            ex = explore.ctypes.data_as(C.c_void_p) if explore is not None else None
            rc = _lib.lib.sfx_runner_phi_test_phase(loop._r, E, 4, 0.03, W_ptr, D, Wb_ptr, ex, None, None, None, None)
            msg = _lib.lib.sfx_last_error().decode()
            assert rc == code and word in msg, (rc, msg)

        def valid():
            w0, b0 = initial_W(E, D, 7)
            W.copy_(w0)
            Wb.copy_(b0)
            _, _, steps = loop.phi_test_phase(W, Wb, horizon=4)
            assert steps.tolist() == [4] * E
            assert not torch.equal(W.cpu(), w0)

        lim = f"1 <= E <= min(16, max_batch = {MAXB})"
        refused(-1, lim, W=torch.zeros(0, D, device=dev), Wb=torch.zeros(0, device=dev))
        valid()
        refused(-1, lim, W=torch.zeros(17, D, device=dev), Wb=torch.zeros(17, device=dev))
        valid()
        refused(-1, "horizon >= 1", horizon=0)
        valid()
        refused(-1, f"w_stride >= d = {D}", W=torch.zeros(E, D - 1, device=dev))
        valid()
        refused(-1, "test_epsilon needs to be in [0, 1]", test_epsilon=1.5)
        refused(-1, "test_epsilon needs to be in [0, 1]", test_epsilon=-0.1)
        valid()
        raw(-1, "non-null", None, Wb.data_ptr())
        raw(-1, "non-null", W.data_ptr(), None)
        valid()
        bad = np.full((E, 4), -1, np.int32)
        bad[2, 3] = A
        raw(-1, f"action >= A = {A}", W.data_ptr(), Wb.data_ptr(), explore=bad)
        with pytest.raises(ValueError, match=f">= A = {A}"):
            loop.phi_test_phase(W, Wb, horizon=4, explore=bad)
        valid()
        # any other schedule (tsf and tsf_phi need the TSF state: G = d, K = 0 serves both)
        eng.tsf_setup(D, 0)
        for t in range(T_):
            eng.tsf_load_g(t, st.g[t])
        eng.tsf_load_h(st.h)
        for sched in ("active", "all", "tsf", "tsf_phi"):
            loop.set_schedule(sched)
            refused(-3, f"phi schedule only, not with schedule {loop.SCHEDULES[sched]} ({sched})")
        # a featurizer (only the active and tsf schedules take one)
        loop.set_schedule("active")
        pre = PreEngine(N_S, D, T_, device=dev)
        try:
            loop.set_featurizer(pre)
            refused(-3, "featurizer")
            loop.set_featurizer(None)
        finally:
            pre.close()
        loop.set_schedule("phi", p_end=0.1)
        valid()
        # a sharded handle; it stays sharded, so this runner takes no valid phase afterwards: the last case on it
        loop.set_schedule("active")
        eng.shard_setup(2 * T_, 0)
        refused(-3, "unsharded")
    finally:
        loop.close()
        eng.close()
    # max_batch below PHIE bounds E as well: E = 9 is refused at max_batch 8, E = 8 runs
    st = make_state("narrow")
    eng = engine_of(st, EV, max_batch=8, tsf=False, phi="mul")
    loop = make_loop(eng, batch=8)
    try:
        with pytest.raises(_lib.SFXError, match=r"1 <= E <= min\(16, max_batch = 8\)"):
            loop.phi_test_phase(torch.zeros(9, D, device=eng.device), torch.zeros(9, device=eng.device), horizon=2)
        W, Wb = (t.to(eng.device) for t in initial_W(8, D, 7))
        assert loop.phi_test_phase(W, Wb, horizon=2)[2].tolist() == [2] * 8
    finally:
        loop.close()
        eng.close()
    # no φ net
    eng = engine_of(st, EV, max_batch=MAXB, tsf=False, phi=None)
    loop = make_loop(eng, schedule="active")
    try:
        with pytest.raises(_lib.SFXError, match="needs a φ net") as ei:
            loop.phi_test_phase(torch.zeros(2, D, device=eng.device), torch.zeros(2, device=eng.device), horizon=2)
        assert "(status -3)" in str(ei.value)
        loop.prefill(16)
        loop.set_task(1)
        loop.run(3)  # still usable
    finally:
        loop.close()
        eng.close()
