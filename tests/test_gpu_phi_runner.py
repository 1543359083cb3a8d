"""GPU checks of the learned-φ agents' training steps in the native env-step runner (sfx_runner_config schedules
5 "phi" and 6 "tsf_phi", sfx_runner_phi_scalars, sfx_runner_phi_losses; csrc/sfx_runner.inc, phi_update_body in
csrc/sfx_phi.inc): agents/sfdqn_phi.py:80-109 over features/deep_phi.py and agents/tsfdqn_phi.py:80-103 over
features/deep_tsf_phi.py.

The exactness claim is test 1's: the runner's steps equal step-by-step calls of sfx_phi_update /
sfx_tsf_phi_update and DeepSF_PHI.GPI_w's biased selection, bit for bit (``==`` / ``torch.equal``), also when
steps were cancelled at their gates and issued again (test 3: no φ kernel may commit under a set cancel word).
Against the CPU restatements (test 2) the bounds are those of tests/test_gpu_phi.py and
tests/test_gpu_tsf_phi.py, imported, with no action-for-action claim: the agents build their Adam afresh every
update, so its steps are close to ±lr·sign(g) and a last-bit difference in a gradient moves a parameter by 2·lr.

Shapes, the smallest that reach every kernel family: ψ Spec(11, 32, 5, 6) (d no multiple of 4, n_in = 23),
T = 3, active task 2, batch 16 (one MFMA row tile) and 20 (two, the second ragged), a target sync every 5
updates (inside the run), p_end 0.1 (γ = 0 rows); φ nets phi_setup(2, 3) (hid 46: the one-workgroup kernels),
phi_setup_dims(132, 3) (wide, 16-byte rows) and phi_setup_dims(131, 1) (wide, scalar-load rows)."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import tsf_phi_ref as TP
from tests.conftest import gpu_available
from tests.test_gpu_engine import rel_close
from tests.test_gpu_phi import check_params as sf_check_params
from tests.test_gpu_tsf_phi import check_params as tsf_check_params
from tests.test_gpu_tsf_phi import engine_of, gpu_state, problem

pytestmark = pytest.mark.gpu

SPEC = R.Spec(11, 32, 5, 6, ("relu", "relu"))
T_, TASK, EV = 3, 2, 5
N_IN = 2 * SPEC.n_s + 1
# name -> (hid, n_mid, engine_of's φ setup)
NETS = {"narrow": (2 * N_IN, 3, "mul"), "w132": (132, 3, "dims"), "w131": (131, 1, "dims")}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def make_state(net_name, seed=31):
    hid, n_mid, _ = NETS[net_name]
    net = TP.Net(SPEC.n_s, SPEC.H, SPEC.A, SPEC.d, SPEC.acts, hid, n_mid)
    return problem(net, T_, seed=seed)


def make_engine(st, net_name, tsf):
    return engine_of(st, EV, max_batch=32, tsf=tsf, phi=NETS[net_name][2])


def make_loop(eng, tsf, B, upd_use_gpi=True, sel_use_gpi=True, **kw):
    from sfx.runner import NativeEnvLoop

    return NativeEnvLoop(eng, batch=B, capacity=200, gamma=0.9, epsilon=0.3, episode_len=11, seed=9,
                         schedule="tsf_phi" if tsf else "phi", use_gpi=sel_use_gpi, upd_use_gpi=upd_use_gpi, p_end=0.1,
                         phi_bias=eng.test_wb, phi_lambda=eng.test_lam, **kw)


def rec_batch(rec):
    return (torch.from_numpy(rec["s"]), torch.from_numpy(rec["a"]), torch.from_numpy(rec["rb"]).view(-1, 1),
            torch.from_numpy(rec["s1"]), torch.from_numpy(rec["gamma"]))


def gpi_w_choice(eng, snext, sel_use_gpi):
    """DeepSF_PHI.GPI_w (features/deep_phi.py) and the agents' greedy branch: eng.gpi's q, plus the bias, argmax."""
    _, q, _, _ = eng.gpi(torch.from_numpy(snext).view(1, -1), w_index=TASK)
    q = q + eng.test_wb[TASK].reshape(1, 1, 1)
    c = int(torch.argmax(torch.max(q, dim=2).values, dim=1)) if sel_use_gpi else TASK
    return c, int(torch.argmax(q[0, c, :]))


def replay_step_by_step(eng2, recs, tsf, upd_use_gpi, sel_use_gpi, final_action):
    """The recorded steps through sfx_phi_update / sfx_tsf_phi_update and the torch-side biased choice; returns
    the last update's losses."""
    fn = eng2.tsf_phi_update if tsf else eng2.phi_update
    last = None
    for k, rec in enumerate(recs):
        assert rec["task"] == TASK
        if rec["have"]:
            s, a, r, s1, gamma = rec_batch(rec)
            last = fn(TASK, s, a, r, s1, gamma, eng2.test_wb[TASK:TASK + 1], eng2.test_lam[TASK:TASK + 1],
                      use_gpi=upd_use_gpi).cpu()
        want = gpi_w_choice(eng2, rec["snext"], sel_use_gpi)
        got = (recs[k + 1]["c"], recs[k + 1]["a_greedy"]) if k + 1 < len(recs) else final_action
        assert got == want, f"step {k}: runner selected {got}, step-by-step calls {want}"
    return last


def assert_same_state(eng, eng2, tsf):
    a, b = gpu_state(eng, T_, tsf), gpu_state(eng2, T_, tsf)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ---- 1. the runner equals step-by-step calls, bit for bit ---------------------------------------
CASES = [  # net, tsf, B, upd_use_gpi, sel_use_gpi
    ("narrow", False, 16, True, True), ("narrow", False, 20, False, False), ("w132", False, 20, True, True),
    ("w131", False, 16, False, True), ("narrow", True, 20, True, True), ("w132", True, 16, False, False),
    ("w132", True, 20, True, True)]


@pytest.mark.parametrize("net,tsf,B,upd_use_gpi,sel_use_gpi", CASES)
def test_runner_equals_step_by_step_calls(net, tsf, B, upd_use_gpi, sel_use_gpi):
    n = 24
    st = make_state(net)
    eng, eng2 = make_engine(st, net, tsf), make_engine(st, net, tsf)
    loop = make_loop(eng, tsf, B, upd_use_gpi, sel_use_gpi)
    loop.prefill(B - 2)  # the first env step runs without a minibatch
    loop.set_task(TASK)
    first = loop.action()
    loop.record(n)
    loop.run(n)
    recs = loop.records()
    assert len(recs) == n and (recs[0]["c"], recs[0]["a_greedy"]) == first
    assert [r["have"] for r in recs[:3]] == [0, 1, 1]
    assert any(r["terminal"] for r in recs) and any((r["gamma"] == 0).any() for r in recs if r["have"])
    assert sum(r["have"] for r in recs) > 2 * EV  # target syncs inside the run
    last = replay_step_by_step(eng2, recs, tsf, upd_use_gpi, sel_use_gpi, loop.action())
    assert_same_state(eng, eng2, tsf)
    assert not torch.equal(eng.phi_get(), st.phi) and not torch.equal(eng.test_wb.cpu(), st.wb)
    assert torch.equal(torch.tensor(loop.phi_losses(), dtype=torch.float32), last), (loop.phi_losses(), last)
    stats = loop.stats()
    assert stats["env_steps"] == n and stats["prelaunched"] > n // 2, stats
    assert stats["ahead_pre_steps"] == 0  # no look-ahead under these schedules
    loop.close()
    eng.close()
    eng2.close()


# ---- 2. against the CPU restatements -------------------------------------------------------------
@pytest.mark.parametrize("net,tsf,B", [("narrow", False, 20), ("w132", False, 16), ("narrow", True, 16),
                                       ("w132", True, 20)])
def test_runner_vs_cpu_restatement(net, tsf, B):
    """The recorded minibatches through oracle/ref_cpu.py phi_update (SF-φ with the reference's net shape,
    hid = 2 n_in) or tests/tsf_phi_ref.py update (TSF-φ; SF-φ on the 132-wide net, which PhiSpec cannot
    describe): tests/test_gpu_phi.py::check_params' / tests/test_gpu_tsf_phi.py::check_params' bounds on the
    final state, the last losses to rtol 1e-4.

    Run length: 6 env steps = 5 updates, the length of the runs those bounds were written for (both files run
    k = 5 updates); the 5th update ends with the target sync, so the synced target heads are among what is
    compared.  params_close scales the size of a flipped entry's error with k (2·lr·k) but not the share of
    flipped entries (max_bad_frac = 2e-3), and that share compounds: a flipped entry changes every later
    gradient.  Measured over the 23 updates of a 24-step run (same seeds), GPU step-by-step calls against the
    restatement: the one-workgroup kernels (hid 46) stay inside the bounds to the end (SF-φ: last losses within
    8e-7, φ net 3.8e-4 of the entries beyond atol + rtol; TSF-φ: none), while the MFMA kernels at hid 132, whose
    reduction order differs from torch's, have at most 2.3e-4 of the φ net and none of the active head beyond
    them through update 7 and then diverge (SF-φ: 1.7e-3 of the active head after 18 updates, 2.3e-2 after 23,
    last losses 1.2e-2 apart; TSF-φ: 1.4e-1 of the active head and 5.6e-1 of the φ net after 23).  The runner adds nothing to that: test 1 holds it to the
    step-by-step calls bit for bit over 24 steps."""
    n = 6
    st = make_state(net, seed=41)
    eng = make_engine(st, net, tsf)
    loop = make_loop(eng, tsf, B)
    loop.prefill(B - 2)
    loop.set_task(TASK)
    loop.record(n)
    loop.run(n)
    recs = [r for r in loop.records() if r["have"]]
    k, got = len(recs), loop.phi_losses()
    assert k == n - 1
    if net == "narrow" and not tsf:
        hid, n_mid, _ = NETS[net]
        ref = R.PhiState(SPEC, R.PhiSpec(SPEC.n_s, SPEC.d, hid // N_IN, n_mid), st.online.clone(), st.target.clone(),
                         st.w.clone(), st.wb.clone(), st.phi.clone(), st.lam.clone())
        for rec in recs:
            s, a, r, s1, gamma = rec_batch(rec)
            want = R.phi_update(ref, (s, a, r, None, s1, gamma), TASK, use_gpi=True, target_update_ev=EV)[:4]
        check = lambda: sf_check_params(eng, ref, T_, k)
    else:
        ref = st.to()
        for rec in recs:
            want = TP.update(ref, rec_batch(rec), TASK, use_gpi=True, target_update_ev=EV, transform=tsf)[:4]
        check = lambda: tsf_check_params(eng, ref, T_, k, tsf=tsf)
    print(f"{net} tsf={tsf} B={B}: {k} updates, losses runner {got} restatement {[float(x) for x in want]}")
    check()
    rel_close(torch.tensor(got), [float(x) for x in want], rtol=1e-4, atol=1e-7)
    loop.close()
    eng.close()


# ---- 3. cancelled steps commit nothing -----------------------------------------------------------
@pytest.mark.parametrize("net,tsf", [("narrow", False), ("w132", False), ("w132", True)])
def test_cancelled_steps_commit_nothing(net, tsf):
    """A gate bound of 10 ns (tests/test_gpu_runner.py::test_runner_gate_timeouts_cancel_and_retry): pre-launched
    steps' gates give up before the host releases them, their launches run under a set cancel word and the steps
    are issued again from the same staged inputs.  The φ net, w, its bias, λ (and g, h) are stepped in place, so a
    single commit under the cancel word would be applied twice: everything must still equal the step-by-step
    calls bit for bit."""
    n, B = 20, 16
    st = make_state(net, seed=51)
    eng, eng2 = make_engine(st, net, tsf), make_engine(st, net, tsf)
    loop = make_loop(eng, tsf, B)
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
    last = replay_step_by_step(eng2, recs, tsf, True, True, loop.action())
    assert_same_state(eng, eng2, tsf)
    assert torch.equal(torch.tensor(loop.phi_losses(), dtype=torch.float32), last)
    # the default bound again: pre-launched steps run without being re-issued
    loop.set_gate_timeout(5.0)
    before = loop.stats()["retried"]
    loop.run(8)
    assert loop.stats()["retried"] == before
    loop.close()
    eng.close()
    eng2.close()


# ---- 4. the biased selection in the runner -------------------------------------------------------
def test_biased_selection_tie_made_by_the_bias_in_the_runner():
    """tests/test_gpu_phi_lockstep.py::test_biased_selection_tie_made_by_the_bias' construction: two q one ulp
    apart, the larger at the later index; a bias of 4 rounds both to 5, so the first index wins, while the
    unbiased selection (a null bias: the active-task schedule) picks the later one.  ψ is pinned through the
    heads' output layer (zero weights, the values in the bias), w = e_0."""
    lo, hi, bias = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)), np.float32(4.0)
    assert hi > lo and np.float32(lo + bias) == np.float32(hi + bias) == np.float32(5.0)
    st = make_state("narrow", seed=61)
    net = st.net
    n_out = net.A * net.d
    for t in range(T_):
        st.online[t, -(n_out * net.H + n_out):] = 0.0
    st.online[0, -n_out + 1 * net.d] = float(lo)   # ψ_0[a = 1][0]
    st.online[1, -n_out + 2 * net.d] = float(hi)   # ψ_1[a = 2][0]
    st.w[:] = 0.0
    st.w[:, 0] = 1.0
    st.wb[:] = float(bias)
    for sel_use_gpi, biased, plain in ((True, (0, 1), (1, 2)), (False, None, None)):
        eng = make_engine(st, "narrow", False)
        loop = make_loop(eng, False, 16, sel_use_gpi=sel_use_gpi)
        loop.set_task(TASK)
        got = loop.action()
        loop.close()
        from sfx.runner import NativeEnvLoop

        ref = NativeEnvLoop(eng, batch=16, capacity=200, seed=9, schedule="active", use_gpi=sel_use_gpi)
        ref.set_task(TASK)
        unbiased = ref.action()
        ref.close()
        if sel_use_gpi:
            assert got == biased and unbiased == plain, (got, unbiased)
        else:  # own-task choice: head 2's q are all zero, with or without the bias: the first action
            assert got == unbiased == (TASK, 0), (got, unbiased)
        eng.close()
    # own-task choice with the tie inside the chosen head: the bias moves the action, not the task
    st.online[TASK, -n_out + 1 * net.d] = float(lo)
    st.online[TASK, -n_out + 3 * net.d] = float(hi)
    eng = make_engine(st, "narrow", False)
    loop = make_loop(eng, False, 16, sel_use_gpi=False)
    loop.set_task(TASK)
    assert loop.action() == (TASK, 1)
    loop.set_schedule("active")
    loop.set_task(TASK)
    assert loop.action() == (TASK, 3)
    loop.close()
    eng.close()


# ---- 5. refusals ---------------------------------------------------------------------------------
def test_refusals_name_the_missing_piece():
    from sfx._lib import SFXError
    from sfx.runner import NativeEnvLoop

    st = make_state("narrow", seed=71)

    def refused(match, fn):
        with pytest.raises(SFXError, match=match) as e:
            fn()
        assert "status -3" in str(e.value)  # SFX_E_STATE

    # no φ setup
    eng = engine_of(st, EV, max_batch=32, tsf=False, phi=None)
    loop = NativeEnvLoop(eng, batch=16, capacity=100, seed=3, schedule="active")
    refused("sfx_runner_phi_scalars", lambda: loop.set_schedule("phi"))
    loop.set_phi_scalars(eng.test_wb, eng.test_lam)
    refused("sfx_phi_setup", lambda: loop.set_schedule("phi"))
    refused("not phi or tsf_phi", loop.phi_losses)
    loop.prefill(16)
    loop.set_task(1)
    loop.run(4)  # still usable, on its earlier schedule
    assert loop.schedule == "active" and loop.stats()["env_steps"] == 4
    loop.close()
    eng.close()
    # a φ setup, but no TSF state / not G = d, K = 0
    eng = make_engine(st, "narrow", False)
    loop = NativeEnvLoop(eng, batch=16, capacity=100, seed=3, schedule="active", phi_bias=eng.test_wb,
                         phi_lambda=eng.test_lam)
    refused(r"sfx_tsf_setup\(G = d, K = 0\)", lambda: loop.set_schedule("tsf_phi"))
    eng.tsf_setup(SPEC.d, 2)
    refused(r"sfx_tsf_setup\(G = d, K = 0\)", lambda: loop.set_schedule("tsf_phi"))
    # device replay on: neither φ schedule configures; under a φ schedule it does not switch on
    loop.set_device_replay(True)
    refused("device replay", lambda: loop.set_schedule("phi"))
    loop.set_device_replay(False)
    loop.set_schedule("phi", p_end=0.1)
    refused("keep the replay on the host", lambda: loop.set_device_replay(True))
    with pytest.raises(ValueError, match="phi_bias"):
        loop.set_phi_scalars(eng.test_wb[:2], eng.test_lam)
    loop.prefill(16)
    loop.set_task(TASK)
    loop.run(6)
    assert loop.stats()["env_steps"] == 6 and len(loop.phi_losses()) == 4
    loop.close()
    eng.close()


def test_refusal_on_a_sharded_handle():
    from sfx._lib import SFXError
    from sfx.runner import NativeEnvLoop

    st = make_state("narrow", seed=72)
    eng = engine_of(st, EV, max_batch=32, tsf=False, phi="mul")
    loop = NativeEnvLoop(eng, batch=16, capacity=100, seed=3, schedule="active", phi_bias=eng.test_wb,
                         phi_lambda=eng.test_lam)
    eng.shard_setup(2 * T_, 0)
    with pytest.raises(SFXError, match="unsharded"):
        loop.set_schedule("phi")
    loop.close()
    eng.close()


def test_python_env_may_return_no_phi():
    """The env callback's φ output is not used under these schedules: a Python env may return None for it."""
    class Env:
        def __init__(self):
            self.t = 0

        def reset(self, task):
            return np.full(SPEC.n_s, 0.1 * task, np.float32)

        def step(self, task, a):
            self.t += 1
            return np.linspace(-1, 1, SPEC.n_s).astype(np.float32) * np.float32(self.t % 5), None, 0.1 * a, self.t % 9 == 0

    st = make_state("narrow", seed=73)
    eng = make_engine(st, "narrow", False)
    loop = make_loop(eng, False, 16, env=Env())
    loop.prefill(16)
    loop.set_task(TASK)
    loop.record(6)
    loop.run(6)
    recs = loop.records()
    assert len(recs) == 6 and all(r["have"] for r in recs) and all((r["phi"] == 0).all() for r in recs)
    assert not torch.equal(eng.phi_get(), st.phi)
    loop.close()
    eng.close()
