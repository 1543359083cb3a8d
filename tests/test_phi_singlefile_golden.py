"""The single-file learned-φ agents' main phase on the CPU (sfdqn_phi.py / tsfdqn_phi.py; sfx/dropin/bind.py): the
binding of their library classes and of tsfdqn_phi.TSFDQN's three methods, the `print_debug` draw of the bound test
mapper, and the committed call logs (tests/golden/calls_*_phi_singlefile.npz, tools/gen_phi_singlefile_golden.py)
held against the oracle.

Fixture tolerances: the logged update_successor / tsf_update calls through oracle/ref_cpu.py at the bounds
tests/test_oracle_golden.py puts on the reference's updates (losses rtol 1e-5 / atol 1e-7, final parameters rtol 1e-4
/ atol 1e-6, target-sync counters exact); each logged φ against tests/pretrain_ref.py's float32 forward of the logged
net on the logged (s, a, s1) at the forward tolerance of tests/test_pretrain_golden.py (rtol 1e-6, atol 1e-7)."""
import random
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import pretrain_ref as PR
from tests.golden import recipe_phi as RP

LOGS = {"sfdqn_phi": "calls_sfdqn_phi_singlefile", "tsfdqn_phi": "calls_tsfdqn_phi_singlefile"}


# ---------------------------------------------------------------------------------------------------------------
# binding
# ---------------------------------------------------------------------------------------------------------------
def fake_module(name):
    """A module shaped like the user's: its own library class, an agent with the methods the binding replaces."""
    m = types.ModuleType(name)
    m.__dict__.update(WHO="user")
    exec(
        "class DeepSF:\n    pass\n"
        "class DeepTSF:\n    pass\n"
        "class Agent:\n"
        "    def pre_train(self, train_tasks, n_samples_pre_train, n_cycles=5):\n        return 'user'\n"
        "    def update_successor(self, transitions, policy_index, use_gpi=True):\n        return 'user'\n"
        "    def get_test_action(self, s_enc, w, omegas):\n        return 'user'\n"
        "    def update_test_reward_mapper(self, w_approx, omegas, optim, task, r, s, a, s1, a1):\n        return 'user'\n"
        "    def test_agent(self, task, test_index):\n        return 'user test_agent'\n"
        "    def train_agent(self):\n        return 'user train_agent'\n"
        "SFDQN = TSFDQN = Agent\n", m.__dict__)
    return m


def test_patch_binds_the_library_classes_and_the_tsf_methods():
    from sfx.dropin import bind
    from sfx.dropin.features import deep_sequential, deep_sequential_tsf

    sf, tsf = fake_module("sfdqn_phi"), fake_module("tsfdqn_phi")
    bind.patch("sfdqn_phi", sf)
    bind.patch("tsfdqn_phi", tsf)
    assert sf.DeepSF is bind.SingleFileDeepSFPhi and issubclass(sf.DeepSF, bind.SingleFileDeepSF)
    assert issubclass(sf.DeepSF, deep_sequential.DeepSF)
    assert tsf.DeepTSF is bind.SingleFileDeepTSFPhi and issubclass(tsf.DeepTSF, bind.SingleFileDeepTSF)
    assert issubclass(tsf.DeepTSF, deep_sequential_tsf.DeepTSF)
    for mod in (sf, tsf):
        assert mod.SFDQN.pre_train is bind.lib_pre_train       # the opening phase stays bound
        assert mod.WHO == "user" and mod.Agent().train_agent() == "user train_agent"
    # sfdqn_phi.SFDQN keeps its own methods (its update goes through DeepSF, its test mapper is torch on one row)
    assert sf.SFDQN().update_successor(None, 0) == "user" and sf.SFDQN().test_agent(None, 0) == "user test_agent"
    T = tsf.TSFDQN
    assert T.update_successor is bind.tsf_update_successor and T.get_test_action is bind.tsf_get_test_action
    assert T.update_test_reward_mapper is bind.tsf_phi_update_test_reward_mapper
    assert T.test_agent.__sfx_bound__ and T.test_agent.__wrapped__(None, None, 0) == "user test_agent"
    for doc in (bind.__doc__, __import__("sfx.dropin", fromlist=["x"]).__doc__):
        assert "keep everything but their opening phase" not in " ".join(doc.split())
        assert "get_w" in doc and "print_debug" in doc


def handle(num_inputs, output_dim, reshape_dim, reshape_axis=1):
    model = torch.nn.Sequential(torch.nn.Linear(num_inputs, 8), torch.nn.Linear(8, 8), torch.nn.ReLU(),
                                torch.nn.Linear(8, output_dim), torch.nn.Unflatten(reshape_axis, reshape_dim))
    return model, torch.nn.MSELoss(), None


HP = dict(RP.AGENT_RUN_TSF_PHI["hp"])


@pytest.mark.parametrize("tsf", [False, True], ids=["DeepSF", "DeepTSF"])
def test_add_training_task_never_asks_for_true_w(tsf):
    """tasks/hopper_phi.py's get_w raises; the reference's classes do not call it and keep no true_w."""
    from sfx.dropin import bind

    task = RP.PhiAgentTask(5, 3, 4, 0, 1, torch.device("cpu"))
    with pytest.raises(NotImplementedError):
        task.get_w()
    if tsf:
        sf = bind.SingleFileDeepTSFPhi(handle, False, target_update_ev=5, hyperparameters=HP)
        extra = (torch.nn.Linear(5, 16), torch.nn.Linear(16, 4))
    else:
        sf = bind.SingleFileDeepSFPhi(handle, target_update_ev=5, hyperparameters=HP)
        extra = ()
    sf.reset()
    assert not hasattr(sf, "true_w")
    torch.manual_seed(3)
    for _ in range(2):
        sf.add_training_task(task, None, *extra)
    assert sf.n_tasks == 2 and len(sf.psi) == 2 and len(sf.fit_w) == 2 and not hasattr(sf, "true_w")
    w = list.__getitem__(sf.fit_w, 1)
    assert isinstance(w, torch.nn.Linear) and tuple(w.weight.shape) == (1, 4)
    assert float(w.weight.detach().abs().max()) <= 0.01
    # the classes they derive from still record it (sfdqn.py:194, :203)
    base = bind.SingleFileDeepTSF(handle, False, hyperparameters=HP) if tsf else bind.SingleFileDeepSF(
        handle, hyperparameters=HP)
    base.reset()
    with pytest.raises(NotImplementedError):
        base.add_training_task(task, None, *extra)


# ---------------------------------------------------------------------------------------------------------------
# the print_debug draw
# ---------------------------------------------------------------------------------------------------------------
class _StubSF:
    def __init__(self):
        self.phis = []

    def tsf_test_update(self, w_approx, omegas, phi, r, s, a, s1, a1, **kw):
        self.phis.append(phi)
        return torch.tensor(3.0), torch.tensor(2.0), torch.tensor(1.0)


def mapper_agent(module_name, print_debug, steps, learnt=True):
    import sys

    from sfx.dropin import bind

    mod = types.ModuleType(module_name)
    if print_debug is not None:
        mod.print_debug = print_debug
    sys.modules[module_name] = mod
    cls = type("TSFDQN", (), {"__module__": module_name,
                              "update_test_reward_mapper": bind.tsf_phi_update_test_reward_mapper})
    agent = cls()
    agent.h_function, agent.sf, agent.gamma, agent.total_training_steps = object(), _StubSF(), 0.9, steps
    agent.hyperparameters = dict(beta_loss_coefficient=1.0, omegas_l1_coefficient=0.0)
    agent.learnt_phi = (lambda s, a, s1: "net φ") if learnt else None
    agent.phi = agent.learnt_phi
    return agent


def call_mapper(agent):
    w = torch.nn.Linear(4, 1, bias=False)
    omegas = torch.ones(1, 2, 1, 1)
    optim = torch.optim.Adam([{"params": w.parameters(), "lr": 1e-3, "weight_decay": 0.0},
                              {"params": [omegas], "lr": 1e-3, "weight_decay": 0.0}])
    task = types.SimpleNamespace(features=lambda s, a, s1: "task φ")
    return agent.update_test_reward_mapper(w, omegas, optim, task, 0.5, None, 1, None, 2)


def test_print_debug_guards_the_random_draw(capsys):
    import sys

    name = "tsfdqn_phi_stand_in"
    try:
        # false (the reference's __main__ value) or absent: Python's random stream is untouched
        for flag in (False, None):
            agent = mapper_agent(name, flag, steps=2000)
            random.seed(5)
            before = random.getstate()
            out = call_mapper(agent)
            assert random.getstate() == before
            assert [float(x) for x in out] == [3.0, 2.0, 1.0] and agent.sf.phis == ["net φ"]
        # true, on a 1000th step: exactly one randint(1, 1000)
        agent = mapper_agent(name, True, steps=3000)
        random.seed(5)
        call_mapper(agent)
        after = random.getstate()
        random.seed(5)
        random.randint(1, 1000)
        assert random.getstate() == after
        # true, off a 1000th step: no draw
        agent = mapper_agent(name, True, steps=3001)
        random.seed(5)
        before = random.getstate()
        call_mapper(agent)
        assert random.getstate() == before
        # without a pre-trained net φ is the task's
        agent = mapper_agent(name, False, steps=1, learnt=False)
        call_mapper(agent)
        assert agent.sf.phis == ["task φ"]
    finally:
        sys.modules.pop(name, None)
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------------------------
# the committed fixtures against the oracle
# ---------------------------------------------------------------------------------------------------------------
def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=rtol, atol=atol)


def recipe_of(stack):
    return RP.AGENT_RUN_TSF_PHI if stack == "tsfdqn_phi" else RP.AGENT_RUN_SEQ_PHI


@pytest.mark.parametrize("stack", sorted(LOGS))
def test_logged_updates_replay_through_the_oracle(golden, stack):
    g, c = golden(LOGS[stack]), recipe_of(stack)
    tsf, hp = stack == "tsfdqn_phi", c["hp"]
    spec = R.Spec(c["n_s"], c["H"], c["A"], c["d"], c["acts"])
    online, target, w = (torch.from_numpy(g["init." + k]).clone() for k in ("online", "target", "w"))
    if tsf:
        gs = R.GSpec(c["n_s"], hp["g_h_function_dims"], 0)
        st = R.TSFState(spec, online, target, w, gspec=gs, g=torch.from_numpy(g["init.g"]).clone(),
                        h=torch.from_numpy(g["init.h"]).clone())
    else:
        st = R.SFState(spec, online, target, w)
    names = [str(n) for n in g["names"]]
    n_upd = 0
    for k, name in enumerate(names):
        if name not in ("update_successor", "tsf_update") or not bool(g[f"c{k}.has_batch"]):
            continue
        batch = tuple(torch.from_numpy(g[f"c{k}.t{i}"]) for i in range(6))
        i, use_gpi = int(g[f"c{k}.policy_index"]), bool(g[f"c{k}.use_gpi"])
        if tsf:
            loss, l1, l2, _ = R.tsf_update(st, batch, i, use_gpi=use_gpi, beta=hp["beta_loss_coefficient"],
                                           lr_sf=hp["learning_rate_sf"], lr_w=hp["learning_rate_w"],
                                           lr_g=hp["learning_rate_g"], lr_h=hp["learning_rate_h"],
                                           target_update_ev=c["target_update_ev"], wd_sf=hp["weight_decay_sf"],
                                           wd_w=hp["weight_decay_w"], wd_g=hp["weight_decay_g"], wd_h=hp["weight_decay_h"])
        else:
            loss, l1, l2, _ = R.sf_update(st, batch, i, use_gpi=use_gpi, lr_sf=hp["learning_rate_sf"],
                                          lr_w=hp["learning_rate_w"], wd_sf=hp["weight_decay_sf"],
                                          wd_w=hp["weight_decay_w"], target_update_ev=c["target_update_ev"])
        close([float(loss), float(l1), float(l2)], g[f"c{k}.losses"], rtol=1e-5, atol=1e-7)
        n_upd += 1
    assert n_upd == c["T_tasks"] * (c["n_samples"] - c["buffer"]["n_batch"] + 1)
    assert n_upd // c["T_tasks"] >= c["target_update_ev"]      # at least one target sync per head
    close(st.online, g["final.online"], rtol=1e-4, atol=1e-6)
    close(st.target, g["final.target"], rtol=1e-4, atol=1e-6)
    assert not np.array_equal(g["final.target"], g["init.target"])
    close(st.w, g["final.w"], rtol=1e-4, atol=1e-6)
    if tsf:
        close(st.g, g["final.g"], rtol=1e-4, atol=1e-6)
        close(st.h, g["final.h"], rtol=1e-4, atol=1e-6)
    assert list(st.since_target) == [int(x) for x in g["final.since_target"]]
    gpi = [k for k, n in enumerate(names) if n == "GPI"]
    assert any(int(g[f"c{k}.task"]) != int(g[f"c{k}.task_index"]) for k in gpi), "no GPI transfer in the log"


@pytest.mark.parametrize("stack", sorted(LOGS))
def test_logged_phi_is_the_logged_net_forward(golden, stack):
    g, c = golden(LOGS[stack]), recipe_of(stack)
    hidden = tuple(int(h) for h in g["final.phi_hidden"])
    assert hidden == (128, 256)     # PhiFunction's widths (sfdqn_phi.py:94-100)
    e = PR.RefEngine(c["n_s"], c["d"], c["T_tasks"], hidden, torch.float32)
    e.load(torch.from_numpy(g["final.phi_net"]))
    calls = [k for k, n in enumerate(str(n) for n in g["names"]) if n == "phi"]
    assert len(calls) >= c["T_tasks"] * c["n_samples"]      # one per env step, one per test-mapper step
    stored = {}
    for k in calls:
        s, a, s1, phi = (g[f"c{k}.{f}"] for f in ("state", "action", "next_state", "phi"))
        assert s.shape == (1, c["n_s"]) and a.shape == () and phi.shape == (1, c["d"])
        want = e.features(torch.from_numpy(s), torch.from_numpy(a).reshape(1), torch.from_numpy(s1))
        close(phi, want, rtol=1e-6, atol=1e-7)
        stored[s.tobytes() + s1.tobytes() + a.tobytes()] = phi
    # the φ rows of the logged minibatches are stored rows: what the runner's featurizer recomputes from (s, a, s1)
    upd = [k for k, n in enumerate(str(n) for n in g["names"]) if n in ("update_successor", "tsf_update")
           and bool(g[f"c{k}.has_batch"])]
    for k in upd[:: max(1, len(upd) // 6)]:
        S, A, PHI, S1 = (g[f"c{k}.t{i}"] for i in (0, 1, 3, 4))
        for b in range(S.shape[0]):
            key = S[b:b + 1].tobytes() + S1[b:b + 1].tobytes() + A[b].tobytes()
            assert key in stored and np.array_equal(stored[key], PHI[b:b + 1]), f"call {k} row {b}"
