"""Host-side checks of the TSF-DQN-with-learned-φ drop-in (no GPU): the install tables, the binding of
agents.tsfdqn_phi and the φ-net geometry that routes to sfx_phi_setup / sfx_phi_setup_dims."""
import types

import pytest
import torch


def _phi_net(n_in, hid, n_mid, d):
    layers = [torch.nn.Linear(n_in, hid), torch.nn.ReLU()]
    for _ in range(n_mid):
        layers += [torch.nn.Linear(hid, hid), torch.nn.ReLU()]
    return torch.nn.Sequential(*layers, torch.nn.Linear(hid, d))


def test_install_tables_name_the_new_modules():
    from sfx import dropin

    assert "features.deep_tsf_phi" in dropin.OURS and "agents.tsfdqn_phi" in dropin.BOUND
    assert "features.deep_tsf_phi" in dropin.__doc__ and "agents.tsfdqn_phi" in dropin.__doc__


def test_phi_geometry_accepts_any_hidden_width():
    from sfx.dropin.features.deep_phi import _phi_geometry

    assert _phi_geometry(_phi_net(13, 26, 3, 12), 6, 12) == (26, 3, 2)       # today's nets: sfx_phi_setup
    assert _phi_geometry(_phi_net(13, 2048, 3, 12), 6, 12) == (2048, 3, None)  # main_tsfdqn_phi_torch.py's
    assert _phi_geometry(_phi_net(13, 136, 1, 12), 6, 12) == (136, 1, None)
    assert _phi_geometry(_phi_net(13, 130, 0, 12), 6, 12) == (130, 0, None)    # a multiple, wider than 128
    with pytest.raises(NotImplementedError):
        _phi_geometry(_phi_net(12, 26, 3, 12), 6, 12)
    with pytest.raises(NotImplementedError):
        _phi_geometry(torch.nn.Sequential(torch.nn.Linear(13, 26), torch.nn.Tanh(), torch.nn.Linear(26, 12)), 6, 12)


def test_binding_of_agents_tsfdqn_phi():
    from sfx.dropin import bind

    calls = []

    class SF:
        def tsf_phi_update(self, *args):
            calls.append(("update",) + args)
            return "losses"

        def sync_tsf_phi_modules(self):
            calls.append(("sync",))

    class TSFDQN_PHI:
        def update_deep_models(self, *a):
            return "user update"

        def test_agent(self, task, test_index):
            calls.append(("test_agent", task, test_index))
            return "user test_agent"

    mod = types.SimpleNamespace(TSFDQN_PHI=TSFDQN_PHI)
    bind.patch("agents.tsfdqn_phi", mod)
    bind.patch("agents.tsfdqn_phi", mod)  # idempotent: test_agent is wrapped once
    agent = TSFDQN_PHI()
    agent.sf, agent.task_index, agent.g_function, agent.h_function = SF(), 1, "g1", "h"
    phis = (("phi_model", None, None), (None, None, None))
    assert agent.update_deep_models(None, phis, 1, "lam", True) is None
    assert agent.update_deep_models("batch", phis, 1, "lam", True) == "losses"
    assert calls == [("update", "batch", "phi_model", "g1", "h", 1, "lam", True)]
    with pytest.raises(NotImplementedError, match="active task"):
        agent.update_deep_models("batch", phis, 0, "lam", True)
    del calls[:]
    assert agent.test_agent("task", 3) == "user test_agent"
    assert calls == [("sync",), ("test_agent", "task", 3)]
    bind.patch("agents.tsfdqn_phi", types.SimpleNamespace())  # a module without the class is left alone


def test_library_interface_without_a_device():
    from sfx.dropin.features.deep_tsf_phi import DeepSF_TSF_PHI
    from tests.golden.recipe import AgentTask, agent_psi_lambda

    sf = DeepSF_TSF_PHI(pytorch_model_handle=agent_psi_lambda(16, ("relu",), 1e-3, "cpu"), target_update_ev=7)
    sf.reset()
    for i in range(2):
        sf.add_training_task(AgentTask(6, 3, 4, i, i, "cpu"))
    assert sf.n_tasks == 2 and sf.target_update_ev == 7
    lin = list.__getitem__(sf.fit_w, 1)
    assert isinstance(lin, torch.nn.Linear) and lin.bias is not None and tuple(lin.weight.shape) == (1, 4)
    for fn in (lambda: sf.update_reward(None, None, 0), lambda: sf.update_successor(None, None, 0)):
        with pytest.raises(Exception, match="shouldn't be used"):
            fn()
    sf.sync_tsf_phi_modules()  # nothing on the device yet: a no-op
