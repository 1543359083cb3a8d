"""GPU checks of the frozen featurizer of the single-file learned-φ agents' main phase (sfdqn_phi.py:482-485, :503;
tsfdqn_phi.py likewise): sfx_pre_features_rows (k_pre_rows, csrc/sfx_pre.h) and sfx_runner_featurizer
(csrc/sfx_runner.inc).

The exactness claims are `torch.equal` ones: row b of an M-row sfx_pre_features_rows call is the one-row
sfx_pre_features call's, and a runner with a featurizer equals step-by-step calls of sfx_pre_features (one row at a
time, as the reference stored φ at append time) followed by sfx_update / sfx_tsf_update.  Against float64 the
forward is held to the bound tests/test_gpu_pretrain.py::test_features applies to sfx_pre_features
(tests/grad_ref.py grad_close).

Shapes: the reference's net (n_s 4, d 12, hidden 128 / 256); a ragged one (n_s 3, d 5, hidden 20 / 7 / 1 / 33: odd
widths, a one-wide layer, four hidden layers, d no multiple of 4); the limits n_s 31 (n_in 63), hidden 256, d 64.
M in {1, 15, 16, 17, 32, 33, 64} covers one to four 16-row tiles and their tails, M = 100 a launch above max_batch.
Runner: ψ Spec(11, 32, 5, 6), T = 2, B 16 (one row tile) and 20 (two, the second ragged), a target sync every 5
updates, p_end 0.1."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import grad_ref as GR
from tests import pretrain_ref as PR
from tests.conftest import gpu_available
from tests.test_gpu_runner import make

pytestmark = pytest.mark.gpu

SHAPES = [(4, 12, (128, 256)), (3, 5, (20, 7, 1, 33)), (31, 64, (256, 256))]
MS = (1, 15, 16, 17, 32, 33, 64)
A_COUNT = 9
ROWS_LIMIT = 65536
_ids = lambda s: f"ns{s[0]}-d{s[1]}-h" + "x".join(map(str, s[2]))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def rows_problem(shape, M=100, seed=0):
    """The net and M rows: row 0 all zeros (action 0), rows 1 and 2 all-negative states, the rest N(0, 1)."""
    n_s, d, hidden = shape
    e = PR.problem(n_s, d, 2, hidden, 7000 + seed)
    gen = torch.Generator().manual_seed(7100 + seed)
    S, a, _, S1 = PR.batch(n_s, A_COUNT, M, gen)
    S[0], S1[0], a[0] = 0.0, 0.0, 0
    S[1:3], S1[1:3] = -S[1:3].abs() - 0.5, -S1[1:3].abs() - 0.5
    return e, S, a, S1


def pre_engine(e, max_batch=64):
    from sfx.pretrain import PreEngine

    eng = PreEngine(e.n_s, e.d, e.T, e.hidden, max_batch=max_batch, device="cuda:0")
    eng.load(e.flat)
    return eng


def features_b(eng, S, a, S1):
    """sfx_pre_features itself (the one-workgroup kernel), B <= max_batch rows."""
    from sfx._lib import check, lib

    S, S1 = eng._dev(S, torch.float32).reshape(-1, eng.n_s), eng._dev(S1, torch.float32).reshape(-1, eng.n_s)
    a = eng._dev(a, torch.long).reshape(-1)
    out = torch.empty(S.shape[0], eng.d, dtype=torch.float32, device=eng.device)
    eng._bind_stream()
    check(lib.sfx_pre_features(eng._h, S.data_ptr(), a.data_ptr(), S1.data_ptr(), S.shape[0], out.data_ptr()),
          "sfx_pre_features")
    return out


def features_rows(eng, S, a, S1):
    from sfx._lib import check, lib

    S, S1 = eng._dev(S, torch.float32).reshape(-1, eng.n_s), eng._dev(S1, torch.float32).reshape(-1, eng.n_s)
    a = eng._dev(a, torch.long).reshape(-1)
    out = torch.full((S.shape[0] + 1, eng.d), 7.5, dtype=torch.float32, device=eng.device)
    eng._bind_stream()
    check(lib.sfx_pre_features_rows(eng._h, S.data_ptr(), a.data_ptr(), S1.data_ptr(), S.shape[0], out.data_ptr()),
          "sfx_pre_features_rows")
    assert bool((out[-1] == 7.5).all()), "a row past M was written"
    return out[:-1]


# ---- 1. the row-tiled forward ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rows_equal_one_row_calls(shape):
    e, S, a, S1 = rows_problem(shape)
    eng = pre_engine(e)
    one = torch.cat([features_b(eng, S[b:b + 1], a[b:b + 1], S1[b:b + 1]) for b in range(100)])
    hidden_on = PR.mlp(e.flat, e.dims[:1], PR.inputs(S, a, S1, torch.float32)) > 0
    assert bool(hidden_on.any()) and bool((~hidden_on).any()), "ReLU must gate both ways"
    for M in MS:
        got = features_rows(eng, S[:M], a[:M], S1[:M])
        assert torch.equal(got, one[:M]), f"M = {M}: rows {(got != one[:M]).any(1).nonzero().view(-1).tolist()} differ " \
                                          "from the one-row sfx_pre_features calls"
        assert torch.equal(got, features_b(eng, S[:M], a[:M], S1[:M])), f"M = {M}: differs from the B = M call"
    got = features_rows(eng, S, a, S1)     # above max_batch = 64
    assert torch.equal(got, one)
    assert torch.equal(features_rows(eng, S, a, S1), got), "two calls from one state differ"
    assert torch.equal(eng.features(S, a, S1), got), "PreEngine.features is not the rows launch"
    # a later offset of the same buffers: tile boundaries move, the rows' bits do not
    assert torch.equal(features_rows(eng, S[7:], a[7:], S1[7:]), one[7:])
    eng.close()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rows_against_float64(shape):
    e, S, a, S1 = rows_problem(shape, seed=1)
    eng = pre_engine(e)
    phi64 = e.clone(torch.float64).features(S, a, S1)
    phi32 = e.features(S, a, S1)
    for M in (17, 100):
        GR.grad_close(f"pre_features_rows {_ids(shape)} M{M}", features_rows(eng, S[:M], a[:M], S1[:M]), phi64[:M],
                      phi32[:M])
    eng.close()


def test_rows_argument_errors():
    from sfx._lib import lib

    e, S, a, S1 = rows_problem(SHAPES[0], 32)
    eng = pre_engine(e, max_batch=32)
    S, a, S1 = S.cuda(), a.cuda(), S1.cuda()
    phi = torch.full((32, 12), 3.0, device="cuda:0")
    ptr = lambda t: t.data_ptr()
    fea = lambda h=eng._h, S_=ptr(S), a_=ptr(a), S1_=ptr(S1), M=32, out=ptr(phi): \
        lib.sfx_pre_features_rows(h, S_, a_, S1_, M, out)
    for call, word in ((lambda: fea(h=None), "null"), (lambda: fea(S_=None), "null"), (lambda: fea(a_=None), "null"),
                       (lambda: fea(S1_=None), "null"), (lambda: fea(out=None), "null"),
                       (lambda: fea(M=0), str(ROWS_LIMIT)), (lambda: fea(M=-1), str(ROWS_LIMIT)),
                       (lambda: fea(M=ROWS_LIMIT + 1), str(ROWS_LIMIT))):
        assert call() == -1
        msg = lib.sfx_last_error().decode()
        assert "sfx_pre_features_rows" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((phi == 3.0).all()), "a refused call wrote φ"
    assert fea() == 0
    eng.close()


# ---- 2. the runner with a featurizer ---------------------------------------------------------------
SPEC = R.Spec(11, 32, 5, 6, ("relu", "relu"))
T_, TASK, EV = 2, 1, 5
HIDDEN = (24, 40)


def tsf_setup(eng):
    K, G = 2, 12
    gs = R.GSpec(SPEC.n_s, G, K)
    gen = torch.Generator().manual_seed(4)
    g = torch.empty(T_, gs.P).uniform_(-0.3, 0.3, generator=gen)
    h = torch.empty(SPEC.d * G + SPEC.d).uniform_(-0.2, 0.2, generator=gen)
    eng.tsf_setup(G, K, 1.0, 1e-3, 0.0, 1e-3, 0.0)
    for t in range(T_):
        eng.tsf_load_g(t, g[t])
    eng.tsf_load_h(h)


def make_engine(schedule):
    eng, _ = make(SPEC, T_, EV, max_batch=32)
    if schedule == "tsf":
        tsf_setup(eng)
    return eng


def make_pre(seed=3, n_s=SPEC.n_s, d=SPEC.d):
    return pre_engine(PR.problem(n_s, d, T_, HIDDEN, 7200 + seed))


def make_loop(eng, schedule, B, upd_use_gpi=True, **kw):
    from sfx.runner import NativeEnvLoop

    return NativeEnvLoop(eng, batch=B, capacity=200, gamma=0.9, epsilon=0.3, episode_len=11, seed=9, schedule=schedule,
                         upd_use_gpi=upd_use_gpi, p_end=0.1, **kw)


def full_state(eng, schedule):
    res = [torch.stack([eng.get_head(t, 0) for t in range(T_)]), torch.stack([eng.get_head(t, 1) for t in range(T_)])]
    res += [torch.stack(eng.get_w(t)) for t in range(T_)]
    for t in range(T_):
        m, v, st = eng.get_adam(t)
        res += [m, v, torch.tensor([st, eng.since_target(t)])]
    if schedule == "tsf":
        res += [torch.stack(eng.tsf_get_g(t)) for t in range(T_)] + [eng.tsf_get_h()]
        res += [torch.stack(eng.tsf_get_h_state(t)) for t in range(T_)]
    return res


def run_loop(schedule, B, upd_use_gpi, n=40, featurizer=True, env=None, ahead=None, monkeypatch=None, pre=None):
    """-> (state, recorded steps, final action, stats) of n steps from the shared initial state."""
    if ahead is not None:
        monkeypatch.setenv("SFX_AHEAD", ahead)
    eng = make_engine(schedule)
    pre = pre or (make_pre() if featurizer else None)
    loop = make_loop(eng, schedule, B, upd_use_gpi, env=env, featurizer=pre)
    loop.prefill(B - 2)     # the first env step runs without a minibatch
    loop.set_task(TASK)
    first = loop.action()
    loop.record(n)
    loop.run(n // 2)
    loop.run(n - n // 2)
    recs = loop.records()
    assert len(recs) == n and (recs[0]["c"], recs[0]["a_greedy"]) == first
    out = (full_state(eng, schedule), recs, loop.action(), loop.stats())
    loop.close()
    eng.close()
    if pre is not None:
        pre.close()
    return out


def step_by_step(schedule, recs, upd_use_gpi, final_action):
    """The recorded steps on a fresh handle: φ = sfx_pre_features of each recorded (s, a, s1) row, one row at a
    time, then sfx_update / sfx_tsf_update, then the select."""
    eng, pre = make_engine(schedule), make_pre()
    upd = eng.tsf_update if schedule == "tsf" else eng.update
    for k, rec in enumerate(recs):
        assert rec["task"] == TASK
        if rec["have"]:
            s, a, s1 = torch.from_numpy(rec["s"]), torch.from_numpy(rec["a"]), torch.from_numpy(rec["s1"])
            phi = torch.cat([features_b(pre, s[b:b + 1], a[b:b + 1], s1[b:b + 1]) for b in range(s.shape[0])])
            upd(TASK, s, a, torch.from_numpy(rec["rb"]).view(-1, 1), phi, s1, torch.from_numpy(rec["gamma"]), upd_use_gpi)
        c, act = (int(x) for x in eng.select_action(torch.from_numpy(rec["snext"]), TASK, True).cpu())
        got = (recs[k + 1]["c"], recs[k + 1]["a_greedy"]) if k + 1 < len(recs) else final_action
        assert got == (c, act), f"step {k}: runner selected {got}, step-by-step calls {(c, act)}"
    state = full_state(eng, schedule)
    eng.close()
    pre.close()
    return state


def assert_equal_states(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: state entry {i} differs"


CASES = [("active", 16, True, "1"), ("active", 20, False, "1"), ("active", 20, True, "0"), ("tsf", 16, True, "1"),
         ("tsf", 20, False, "1"), ("tsf", 20, True, "0")]


@pytest.mark.parametrize("schedule,B,upd_use_gpi,ahead", CASES)
def test_runner_equals_step_by_step_calls(schedule, B, upd_use_gpi, ahead, monkeypatch):
    n = 40
    state, recs, final, stats = run_loop(schedule, B, upd_use_gpi, n, ahead=ahead, monkeypatch=monkeypatch)
    assert [r["have"] for r in recs[:3]] == [0, 1, 1]
    assert any(r["terminal"] for r in recs) and any((r["gamma"] == 0).any() for r in recs if r["have"])
    assert sum(r["have"] for r in recs) > 2 * EV     # target syncs inside the run
    assert_equal_states(state, step_by_step(schedule, recs, upd_use_gpi, final), f"{schedule} B{B}")
    assert stats["env_steps"] == n and stats["prelaunched"] > n // 2 and stats["nonfinite_steps"] == 0, stats
    # the active schedule keeps its look-ahead under a featurizer, the TSF one does not look ahead
    if schedule == "active" and ahead == "1":
        assert stats["ahead_pre_steps"] > 0, stats
    else:
        assert stats["ahead_pre_steps"] == 0, stats


@pytest.mark.parametrize("schedule", ["active", "tsf"])
def test_cancelled_steps_with_a_featurizer(schedule):
    """A gate bound of 10 ns (tests/test_gpu_runner.py::test_runner_gate_timeouts_cancel_and_retry): pre-launched steps'
    gates give up, their launches -- k_pre_rows among them -- run under a set cancel word and the steps are issued
    again from the same staged inputs.  Everything must still equal the step-by-step calls bit for bit."""
    n, B = 20, 16
    eng, pre = make_engine(schedule), make_pre()
    loop = make_loop(eng, schedule, B, featurizer=pre)
    loop.prefill(B)
    loop.set_task(TASK)
    loop.set_gate_timeout(1e-8)
    loop.record(4 * n)
    for _ in range(4):
        loop.run(n)
        stats = loop.stats()
        if stats["retried"] > 0:
            break
    assert stats["retried"] > 0 and stats["prelaunched"] > 0, stats
    recs = loop.records()
    assert len(recs) == stats["env_steps"]
    state, final = full_state(eng, schedule), loop.action()
    loop.close()
    eng.close()
    pre.close()
    assert_equal_states(state, step_by_step(schedule, recs, True, final), f"{schedule}, cancelled steps")


class Env:
    """tasks/task.py-shaped host env; `phi`: what step returns for φ ("rows": finite rows, None, "nan")."""

    def __init__(self, n_s, d, phi):
        self.n_s, self.d, self.phi, self.t = n_s, d, phi, 0

    def reset(self, task):
        return np.full(self.n_s, 0.1 * (task + 1), np.float32)

    def step(self, task, a):
        self.t += 1
        s1 = (np.linspace(-1, 1, self.n_s) * (self.t % 5 - 2) + 0.01 * a).astype(np.float32)
        phi = {"rows": np.full(self.d, 0.01 * (self.t % 7), np.float32), "none": None,
               "nan": np.full(self.d, np.nan, np.float32)}[self.phi]
        return s1, phi, 0.1 * (self.t % 3), self.t % 9 == 0


@pytest.mark.parametrize("schedule", ["active", "tsf"])
def test_env_phi_is_never_read(schedule):
    runs = {k: run_loop(schedule, 16, True, 30, env=Env(SPEC.n_s, SPEC.d, k)) for k in ("rows", "none", "nan")}
    base = runs["rows"]
    for k in ("none", "nan"):
        state, recs, final, stats = runs[k]
        assert_equal_states(state, base[0], f"{schedule}, env φ {k}")
        assert [(r["c"], r["a_greedy"], r["a_taken"]) for r in recs] == \
               [(r["c"], r["a_greedy"], r["a_taken"]) for r in base[1]] and final == base[2]
        assert stats["nonfinite_steps"] == 0, stats
    assert any(np.isnan(r["phi"]).any() for r in runs["nan"][1] if r["have"]), "the NaN rows did reach the staging"
    assert_equal_states(base[0], step_by_step(schedule, base[1], True, base[2]), f"{schedule}, python env")


def test_refusals():
    from sfx._lib import SFXError, lib

    def refused(fn, status, *words):
        with pytest.raises(SFXError) as ei:
            fn()
        msg = str(ei.value)
        assert f"(status {status})" in msg and all(w in msg for w in words), msg

    STATE, ARG = -3, -1
    eng, pre = make_engine("active"), make_pre()
    eng.phi_setup(2, 3)
    bias, lam = torch.zeros(T_, device="cuda:0"), torch.ones(T_, device="cuda:0")
    # the featurizer second
    for schedule in ("all", "phi"):
        loop = make_loop(eng, schedule, 16, phi_bias=bias, phi_lambda=lam)
        refused(lambda: loop.set_featurizer(pre), STATE, "sfx_runner_featurizer", f"({schedule})")
        loop.close()
    # the schedule second ("sharded" only in this order: without a communicator no runner is ever configured to it)
    loop = make_loop(eng, "active", 16, featurizer=pre, phi_bias=bias, phi_lambda=lam)
    for schedule in ("all", "phi", "tsf_phi", "sharded"):
        refused(lambda: loop.set_schedule(schedule), STATE, "sfx_runner_config", "featurizer", f"({schedule})")
    loop.set_schedule("active")
    # device replay, both orders
    refused(lambda: loop.set_device_replay(True), STATE, "sfx_runner_device_replay", "featurizer")
    loop.set_featurizer(None)
    loop.set_device_replay(True)
    refused(lambda: loop.set_featurizer(pre), STATE, "sfx_runner_featurizer", "device replay")
    loop.set_device_replay(False)
    loop.set_featurizer(pre)
    # n_s / d mismatch: both values named
    for kw, words in ((dict(n_s=SPEC.n_s + 1), ("n_s = 12", "n_s = 11")), (dict(d=SPEC.d + 2), ("d = 8", "d = 6"))):
        other = make_pre(**kw)
        refused(lambda: loop.set_featurizer(other), ARG, "sfx_runner_featurizer", *words)
        other.close()
    assert lib.sfx_runner_featurizer(None, pre.handle) == ARG
    loop.close()
    eng.close()
    pre.close()


@pytest.mark.parametrize("schedule", ["active", "tsf"])
def test_cleared_featurizer_restores_the_plain_runner(schedule):
    """Set, then cleared with NULL before the first step: bit for bit a runner that never had one (φ from the env)."""
    def run(touch):
        eng = make_engine(schedule)
        pre = make_pre()
        loop = make_loop(eng, schedule, 16)
        if touch:
            loop.set_featurizer(pre)
            loop.set_featurizer(None)
        loop.prefill(14)
        loop.set_task(TASK)
        loop.record(30)
        loop.run(30)
        out = (full_state(eng, schedule), [(r["c"], r["a_greedy"], r["a_taken"]) for r in loop.records()], loop.action(),
               loop.stats())
        loop.close()
        eng.close()
        pre.close()
        return out

    a, b = run(True), run(False)
    assert_equal_states(a[0], b[0], schedule)
    assert a[1] == b[1] and a[2] == b[2]
    assert a[3]["ahead_pre_steps"] == b[3]["ahead_pre_steps"] > 0
