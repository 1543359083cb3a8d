"""DeepSF_TSF_PHI on the GPU (the interface of features/deep_tsf_phi.py:9-164, the library of
main_tsfdqn_phi_torch.py with agents/tsfdqn_phi.py): TSF-DQN with a learned φ.

The ψ heads, their targets and each task's reward model (an nn.Linear(d, 1) WITH bias,
features/deep_tsf_phi.py:156) live in a libsfx engine, as in DeepSF_PHI.  The update is the agent's
(TSFDQN_PHI.update_deep_models, agents/tsfdqn_phi.py:180-288); sfx.dropin.bind turns it into
``tsf_phi_update``, one libsfx call (sfx_tsf_phi_update): φ̃ = φ_net(s ⊕ a ⊕ s') ⊙ (h(g_i(s)) + h(g_i(s'))),
GPI / own-ψ next actions, targets φ̃ + γ ψ⁻_i(s')[a'] that carry φ̃'s gradient, loss = MSE(w_i(φ̃), r) +
λ_i MSE(ψ_i(s), merged), gradients clamped to [-1, 1], one freshly built Adam step (lr 1e-3, as the
reference hard-codes) on ψ_i, the φ net, g_i, h, w_i and its bias, ascent on λ_i, clamped to [1e-2, 1e6].
The agent's φ net (main_tsfdqn_phi_torch.py's phi_model_lambda: hidden width 2048, the wide kernels of
csrc/sfx_phiw.h), the task's g_i and the shared h are loaded into the engine the first time an update
hands them in, and train there; ``sync_tsf_phi_modules`` copies them back into the agent's modules
(sfx.dropin.bind calls it before the agent's test episodes).

The test phase (agents/tsfdqn_phi.py:381-505) runs in the library too: ``tsf_phi_test_action`` is
get_test_action's greedy branch (sfx_tsf_phi_test_action), ``tsf_phi_test_update`` is update_target_models
(sfx_tsf_phi_test_update) on the agent's own ``omegas``, the test task's nn.Linear(d, 1) and its loss
coefficient, all three updated in place.  A test step may come before the first training update: it loads
the agent's φ net, h and EVERY g_t the engine has not seen yet.
"""
from __future__ import annotations

import torch

from .deep import _flat, _unflat_into
from .deep_phi import LR, DeepSF_PHI, _is_linear, _on_engine_device

# one workgroup of k_tsfphi_test_* (csrc/sfx_phitest.h): d, A, A d, T d, A T d
TEST_LIMITS = (64, 64, 1024, 1024, 4096)


class DeepSF_TSF_PHI(DeepSF_PHI):
    def __init__(self, pytorch_model_handle, *args, target_update_ev=1000, **kwargs):
        super().__init__(pytorch_model_handle, *args, target_update_ev=target_update_ev, **kwargs)

    def reset(self):
        super().reset()
        self._g_mods = {}
        self._h_mod = None

    # ------------------------------------------------------------------ ψ
    def get_next_successor(self, state, policy_index):
        return self.get_next_successors(state)[:, policy_index]

    def get_next_successors(self, state):
        s = self._state(state)
        eng = self._engine(s.shape[0])
        self._flush()
        return eng.successors(s, which=1).to(self._out_device())

    def update_reward(self, phi, r, task_index, exact=False):
        raise Exception("This function shouldn't be used")

    def update_successor(self, transitions, phis_models, policy_index):
        raise Exception("This function shouldn't be used")

    # ------------------------------------------------------------------ training
    def _tsf_phi_engine(self, phi_model, g_i, h, policy_index, batch):
        fresh = self._phi_model is None
        eng = self._phi_engine(phi_model, batch)
        d, n_s = self.n_features, self.inputs
        if fresh:
            if not isinstance(h, torch.nn.Linear) or h.bias is None or (h.in_features, h.out_features) != (d, d):
                raise NotImplementedError(f"sfx DeepSF_TSF_PHI: h must be nn.Linear(d, d) with bias; got {h}")
            eng.tsf_setup(d, 0, 1.0, LR, 0.0, LR, 0.0)
            eng.tsf_load_h(_flat(h))
            self._h_mod = h
        elif h is not self._h_mod:
            raise NotImplementedError("sfx DeepSF_TSF_PHI: one shared h per library")
        known = self._g_mods.get(policy_index)
        if known is None:
            if not isinstance(g_i, torch.nn.Linear) or g_i.bias is None or \
                    (g_i.in_features, g_i.out_features) != (n_s, d):
                raise NotImplementedError(f"sfx DeepSF_TSF_PHI: g_i must be nn.Linear(n_s, d) with bias; got {g_i}")
            eng.tsf_load_g(policy_index, _flat(g_i))
            self._g_mods[policy_index] = g_i
        elif g_i is not known:
            raise NotImplementedError("sfx DeepSF_TSF_PHI: one g_i per task")
        return eng

    def tsf_phi_update(self, transitions, phi_model, g_i, h, policy_index, loss_coefficient, use_gpi):
        """agents/tsfdqn_phi.py:180-288 -> (loss, psi_loss, phi_loss, loss_coefficient)."""
        states, actions, rs, _, next_states, gammas = transitions
        eng = self._tsf_phi_engine(phi_model, g_i, h, policy_index, len(gammas))
        self._flush()
        bias_mod = list.__getitem__(self.fit_w, policy_index).bias
        bias, bias_staged = self._dev_scalar(bias_mod.data, eng)
        lam, lam_staged = self._dev_scalar(loss_coefficient.data, eng)
        losses = eng.tsf_phi_update(policy_index, states, actions, rs, next_states, gammas, bias, lam,
                                    use_gpi=use_gpi)
        self._phi_updates += 1
        with torch.no_grad():
            if bias_staged:
                bias_mod.copy_(bias.view_as(bias_mod))
            if lam_staged:
                loss_coefficient.copy_(lam.view_as(loss_coefficient))
        self._host_stale = True
        dev = self._out_device()
        loss, psi_loss, phi_loss = (x.reshape(1).to(dev) for x in (losses[0], losses[1], losses[2]))
        return loss, psi_loss, phi_loss, loss_coefficient

    def sync_tsf_phi_modules(self):
        """Copy the device's φ net, g_i and h into the agent's modules."""
        if not self._phi_ready():
            return
        self.sync_phi_module()
        for t, g in self._g_mods.items():
            _unflat_into(g, self._eng.tsf_get_g(t)[0])
        if self._h_mod is not None:
            _unflat_into(self._h_mod, self._eng.tsf_get_h())

    # ------------------------------------------------------------------ test phase
    def tsf_phi_test_supported(self, agent, w_approx, lam=None) -> bool:
        """The library can run this agent's test step: ``omegas`` an nn.Linear(T d, d) and w_approx an
        nn.Linear(d, 1), both with bias and on the engine's device, λ a one-element float32 tensor there, g_t
        and h plain Linears, a φ net the setups take, shapes within k_tsfphi_test_*'s.  Pure Python: no
        library call.  ``omegas`` is read from the agent each time: add_training_task re-creates it."""
        T, d, A, dev = self.n_tasks, self.n_features, self.n_actions, self._test_device()
        if T == 0 or d > TEST_LIMITS[0] or A > TEST_LIMITS[1] or A * d > TEST_LIMITS[2] or T * d > TEST_LIMITS[3] \
                or A * T * d > TEST_LIMITS[4]:
            return False
        gs, h = getattr(agent, "g_functions", None), getattr(agent, "h_function", None)
        ok = _is_linear(getattr(agent, "omegas", None), T * d, d, dev) and _is_linear(w_approx, d, 1, dev)
        ok = ok and (lam is None or (_on_engine_device(lam, dev) and lam.numel() == 1))
        ok = ok and isinstance(h, torch.nn.Linear) and h.bias is not None and (h.in_features, h.out_features) == (d, d)
        ok = ok and gs is not None and len(gs) == T and all(
            isinstance(g, torch.nn.Linear) and g.bias is not None and (g.in_features, g.out_features) == (self.inputs, d)
            for g in gs)
        return bool(ok) and self._phi_fits(agent.phi[0][0])

    def _tsf_phi_test_engine(self, agent):
        """The engine with the agent's φ net, h and every g_t loaded (those no update has handed in yet)."""
        pm, gs, h = agent.phi[0][0], agent.g_functions, agent.h_function
        if self._phi_model is pm and self._h_mod is h and len(self._g_mods) == len(gs) and \
                all(self._g_mods.get(t) is g for t, g in enumerate(gs)):
            return self._phi_engine(pm, 1)
        eng = None
        for t, g in enumerate(gs):
            eng = self._tsf_phi_engine(pm, g, h, t, 1)
        return eng

    def tsf_phi_test_action(self, agent, s_enc, w_approx):
        """agents/tsfdqn_phi.py:381-397, the greedy branch -> a 0-dim int64 tensor."""
        eng = self._tsf_phi_test_engine(agent)
        self._flush()
        om = agent.omegas
        a = eng.tsf_phi_test_action(torch.as_tensor(s_enc).reshape(-1), om.weight.data, om.bias.data,
                                    w_approx.weight.data, w_approx.bias.data)
        return a.to(self._out_device())

    def tsf_phi_test_update(self, agent, w_approx, lam, r, s_enc, a, s1_enc):
        """agents/tsfdqn_phi.py:434-505 update_target_models -> (loss [1], psi_loss, phi_loss); ``agent.omegas``,
        w_approx and λ updated in place."""
        eng = self._tsf_phi_test_engine(agent)
        self._flush()
        om = agent.omegas
        lo = eng.tsf_phi_test_update(s_enc, a, float(r), s1_enc, float(agent.gamma), om.weight.data, om.bias.data,
                                     w_approx.weight.data, w_approx.bias.data, lam.data)
        dev = self._out_device()
        return lo[0:1].to(dev), lo[1].to(dev), lo[2].to(dev)
