"""Binding of the reference modules that hold the SF library inside the same file as an agent.

The single-file scripts define their library next to their agent: ``sfdqn.DeepSF``
(sfdqn.py:94-371), ``tsfdqn.DeepTSF`` / ``tsfdqn_nf.DeepTSF`` (tsfdqn.py:93-326), and the TSF
agents carry the update itself (``TSFDQN.update_successor``, tsfdqn.py:588-709,
tsfdqn_nf.py:620-741, agents/tsfdqn_sequential.py:123-252).  ``sfx.dropin.install()`` lets the
user's own modules load unchanged and then applies ``patch``: the library classes become
sfx's, the TSF agents' update_successor becomes one libsfx call (DeepTSF.tsf_update), and their
test-task methods get_test_action / update_test_reward_mapper (tsfdqn.py:859-997, SURVEY §8f
rank 1) become libsfx calls too (DeepTSF.tsf_test_action / tsf_test_update), drawing from
Python's random module exactly where the reference does.  ``agents.tsfdqn_phi``'s
``TSFDQN_PHI.update_deep_models`` (:180-288, TSF-DQN with a learned φ) becomes one libsfx call
(DeepSF_TSF_PHI.tsf_phi_update), and its test phase's get_test_action / update_target_models
(:381-397, :434-505) become libsfx calls on the agent's own ``omegas``, the test task's reward model
and loss coefficient (DeepSF_TSF_PHI.tsf_phi_test_action / tsf_phi_test_update);
``agents.sfdqn_phi``'s update_test_reward_mapper (:263-305) likewise (DeepSF_PHI.phi_test_update).
Where the agent's modules are not the shapes the library runs, those methods fall back to the
agent's own torch code, after the device's φ net, g_i and h are copied back into its modules -- as
``test_agent`` is wrapped to do once per test episode.

The single-file learned-φ agents ``sfdqn_phi`` / ``tsfdqn_phi`` are bound whole.  Their opening phase
``SFDQN.pre_train`` (sfdqn_phi.py:800-873) / ``TSFDQN.pre_train`` (tsfdqn_phi.py:1036-1109) becomes
``sfx.pretrain.pre_train``, which leaves ``self.learnt_phi`` a frozen net on the device (sfx.pretrain.LearntPhi).
Their main phase is the other single-file agents' but for where φ comes from -- ``self.phi = self.learnt_phi``
(sfdqn_phi.py:482-485), ``phi = self.phi(s_enc, a, s1_enc)`` (:503) -- so ``sfdqn_phi.DeepSF`` /
``tsfdqn_phi.DeepTSF`` become subclasses of the single-file library classes that never call ``task.get_w()`` and
keep no ``true_w`` (tasks/hopper_phi.py's get_w raises; the reference's classes dropped both), and
``tsfdqn_phi.TSFDQN``'s update_successor / get_test_action / update_test_reward_mapper are bound as
``tsfdqn.TSFDQN``'s are, with the reference's two differences: the mapper's φ is ``self.phi(s, a, s1)`` when
``self.learnt_phi`` is set, and its diagnostic block -- with the ``random.randint(1, 1000)`` draw -- runs only when
the module's ``print_debug`` is true.  The stored φ reaches update_successor as data (``phis.detach()``,
sfdqn_phi.py:369-371), which is how sfx_update / sfx_tsf_update take it.  The agents' ``test_agent`` loops (10
episodes per test task), ``sfdqn_phi.SFDQN``'s own test mapper and everything else stay the user's; sfx.lockstep
does not cover these two agents.
"""
from __future__ import annotations

import functools
import random

import torch

from .features import deep_sequential as _seq
from .features import deep_sequential_tsf as _tsf


class SingleFileDeepSF(_seq.DeepSF):
    """sfdqn.py:94-371's constructor: (pytorch_model_handle, use_true_reward=False, target_update_ev=1000)."""

    def __init__(self, pytorch_model_handle, use_true_reward=False, target_update_ev=1000, **kwargs):
        super().__init__(pytorch_model_handle, target_update_ev=target_update_ev, use_true_reward=use_true_reward,
                         **kwargs)


class SingleFileDeepTSF(_tsf.DeepTSF):
    """tsfdqn.py:93-326 / tsfdqn_nf.py:95-327's constructor: ``use_true_reward`` is positional."""

    def __init__(self, pytorch_model_handle, use_true_reward, target_update_ev=1000, **kwargs):
        super().__init__(pytorch_model_handle, target_update_ev=target_update_ev, use_true_reward=use_true_reward,
                         **kwargs)


class _NoTrueW:
    """sfdqn_phi.py:161, :224, :232 / tsfdqn_phi.py likewise: no ``true_w`` list, no ``task.get_w()`` call."""

    def reset(self):
        super().reset()
        del self.true_w

    def _note_true_w(self, task):
        pass


class SingleFileDeepSFPhi(_NoTrueW, SingleFileDeepSF):
    """sfdqn_phi.py's DeepSF: sfdqn.py's without the true reward weights; φ arrives in the transitions as data."""


class SingleFileDeepTSFPhi(_NoTrueW, SingleFileDeepTSF):
    """tsfdqn_phi.py's DeepTSF: tsfdqn.py's without the true reward weights."""


def tsf_update_successor(self, transitions, policy_index, use_gpi=True):
    """TSFDQN.update_successor (tsfdqn.py:588-709) as one device call: GPI (or own-ψ) next actions,
    φ̃ = (h(g_i(s)) + h(g_i(s'))) ⊙ φ, TD target, l1 + β l2, Adam over {ψ_i, w_i, g_i, h}, target
    sync -- with the agent's g_i and h, which the library received in add_training_task.
    Returns (loss, l1, l2) as the reference does."""
    if transitions is None:
        return None
    if self.h_function is None:
        raise Exception("Affine Function (h) is not initialized")
    return self.sf.tsf_update(transitions, policy_index, use_gpi,
                              beta=self.hyperparameters["beta_loss_coefficient"])


def tsf_get_test_action(self, s_enc, w, omegas):
    """TSFDQN.get_test_action (tsfdqn.py:859-870): the same ε draw from Python's random module;
    the greedy branch argmax_a w·Σ_t ω̂_t ψ_t(s)[a] is one library call (sfx_tsf_test_action)."""
    with torch.no_grad():
        if random.random() <= self.test_epsilon:
            return torch.tensor(random.randrange(self.n_actions)).to(self.device)
        return self.sf.tsf_test_action(s_enc, w, omegas)


def prints_phi_shape(agent) -> bool:
    """agents/tsfdqn_sequential.py:443 prints ``Phi values {phi.shape}`` on every call of its
    reward mapper; tsfdqn.py / tsfdqn_nf.py do not."""
    return type(agent).__module__.split(".")[-1] == "tsfdqn_sequential"


def tsf_update_test_reward_mapper(self, w_approx, omegas, optim, task, r, s, a, s1, a1):
    """TSFDQN.update_test_reward_mapper (tsfdqn.py:917-997, agents/tsfdqn_sequential.py:435-520) as
    one library call (sfx_tsf_test_update): φ from the user's task, the learning rates and weight
    decays read from the agent's optimizer groups (its LambdaLR keeps decaying ω's), the Adam step
    on the device.  Returns (loss, l2, l1) as the reference does.

    Console output: agents/tsfdqn_sequential.py's unconditional ``Phi values`` line is printed as
    the reference does; the occasional diagnostic block (every 1000th training step, when
    ``random.randint(1, 1000) < 10``) draws from the same random stream but prints ONE line (the
    task's ω and w) instead of the reference's block of intermediate tensors, and ``omegas.grad`` /
    ``w_approx.weight.grad`` are not populated (the gradients live on the device only)."""
    if self.h_function is None:
        raise Exception('Affine Function (h) is not initialized')
    phi = task.features(s, a, s1)
    if prints_phi_shape(self):
        print(f'Phi values {phi.shape}')
    gw, go = optim.param_groups[0], optim.param_groups[1]
    for grp in (gw, go):
        if tuple(grp.get("betas", (0.9, 0.999))) != (0.9, 0.999) or grp.get("eps", 1e-8) != 1e-8:
            raise NotImplementedError("sfx: the test reward mapper's Adam runs with betas (0.9, 0.999), eps 1e-8")
    hp = self.hyperparameters
    loss, l2, l1 = self.sf.tsf_test_update(w_approx, omegas, phi, r, s, a, s1, a1, gamma=self.gamma,
                                           beta=hp['beta_loss_coefficient'], lasso=hp['omegas_l1_coefficient'],
                                           lr_w=gw['lr'], wd_w=gw['weight_decay'], lr_o=go['lr'],
                                           wd_o=go['weight_decay'])
    # the reference's occasional diagnostic print draws from the same random stream
    if self.total_training_steps % 1000 == 0 and random.randint(1, 1000) < 10:
        print(f'Target Task {task} omegas {omegas.detach()} weights {w_approx.weight.detach()}')
    return loss, l2, l1


def _print_debug(agent) -> bool:
    """The ``print_debug`` global of the agent's own module (tsfdqn_phi.py:1160, set by its __main__ block)."""
    import sys

    return bool(getattr(sys.modules.get(type(agent).__module__), "print_debug", False))


def tsf_phi_update_test_reward_mapper(self, w_approx, omegas, optim, task, r, s, a, s1, a1):
    """tsfdqn_phi.py's TSFDQN.update_test_reward_mapper: tsf_update_test_reward_mapper with the reference's two
    differences -- φ is ``self.phi(s, a, s1)`` when ``self.learnt_phi`` is set (the frozen net, one library call),
    else ``task.features``; the diagnostic block and its ``random.randint(1, 1000)`` draw sit under the module's
    ``print_debug``, so Python's random stream is the reference's.  Returns (loss, l2, l1)."""
    if self.h_function is None:
        raise Exception('Affine Function (h) is not initialized')
    with torch.no_grad():
        phi = task.features(s, a, s1) if self.learnt_phi is None else self.phi(s, a, s1)
    gw, go = optim.param_groups[0], optim.param_groups[1]
    for grp in (gw, go):
        if tuple(grp.get("betas", (0.9, 0.999))) != (0.9, 0.999) or grp.get("eps", 1e-8) != 1e-8:
            raise NotImplementedError("sfx: the test reward mapper's Adam runs with betas (0.9, 0.999), eps 1e-8")
    hp = self.hyperparameters
    loss, l2, l1 = self.sf.tsf_test_update(w_approx, omegas, phi, r, s, a, s1, a1, gamma=self.gamma,
                                           beta=hp['beta_loss_coefficient'], lasso=hp['omegas_l1_coefficient'],
                                           lr_w=gw['lr'], wd_w=gw['weight_decay'], lr_o=go['lr'],
                                           wd_o=go['weight_decay'])
    if _print_debug(self):
        if self.total_training_steps % 1000 == 0 and random.randint(1, 1000) < 10:
            print(f'Target Task {task} omegas {omegas.detach()} weights {w_approx.weight.detach()}')
    return loss, l2, l1


def _synced(method):
    """Run the agent's own method after the device's g_i / h are copied into its modules (the test
    tasks' reward mapper, tsfdqn.py:874-997, reads them in torch)."""
    @functools.wraps(method)
    def run(self, *args, **kwargs):
        sync = getattr(self.sf, "sync_tsf_modules", None)
        if sync is not None:
            sync()
        return method(self, *args, **kwargs)

    run.__sfx_bound__ = True
    return run


def patch_tsf_agent(cls, mapper=tsf_update_test_reward_mapper) -> None:
    cls.update_successor = tsf_update_successor
    if hasattr(cls, "get_test_action") and hasattr(cls, "update_test_reward_mapper"):
        cls.get_test_action = tsf_get_test_action
        cls.update_test_reward_mapper = mapper
    for name in ("test_agent",):
        m = getattr(cls, name, None)
        if m is not None and not getattr(m, "__sfx_bound__", False):
            setattr(cls, name, _synced(m))


def _phi_synced(method):
    """Run the agent's own method after the device's φ net is copied into the agent's module (its
    test reward mapper, agents/sfdqn_phi.py update_test_reward_mapper, runs φ in torch)."""
    @functools.wraps(method)
    def run(self, *args, **kwargs):
        sync = getattr(self.sf, "sync_phi_module", None)
        if sync is not None:
            sync()
        return method(self, *args, **kwargs)

    run.__sfx_bound__ = True
    return run


def tsf_phi_update_deep_models(self, transitions, phis_model, policy_index, loss_coefficient, use_gpi):
    """TSFDQN_PHI.update_deep_models (agents/tsfdqn_phi.py:180-288) as one device call
    (sfx_tsf_phi_update) with the agent's φ net, its active task's g_i and the shared h.  The reference
    transforms with the ACTIVE task's g whatever policy_index says, and none of its callers passes
    another policy: anything else is refused.  Returns (loss, psi_loss, phi_loss, loss_coefficient)."""
    if transitions is None:
        return None
    if policy_index != self.task_index:
        raise NotImplementedError("sfx TSFDQN_PHI.update_deep_models: policy_index must be the active task "
                                  f"({self.task_index}), got {policy_index}")
    (phi_model, _, _), _ = phis_model
    return self.sf.tsf_phi_update(transitions, phi_model, self.g_function, self.h_function, policy_index,
                                  loss_coefficient, use_gpi)


def _tsf_phi_synced(method):
    """Run the agent's own method after the device's φ net, g_i and h are copied into its modules (the
    test phase, agents/tsfdqn_phi.py:381-505, runs them in torch)."""
    @functools.wraps(method)
    def run(self, *args, **kwargs):
        sync = getattr(self.sf, "sync_tsf_phi_modules", None)
        if sync is not None:
            sync()
        return method(self, *args, **kwargs)

    run.__sfx_bound__ = True
    return run


def _fallback(self, sync_name):
    """Before the agent's own torch code runs: the device's state into its modules, if an update ran since."""
    sync = getattr(self.sf, sync_name, None)
    if sync is not None:
        self.sf.sync_if_stale(sync)


def bind_tsf_phi_test(cls) -> None:
    """TSFDQN_PHI.get_test_action (agents/tsfdqn_phi.py:381-397) and update_target_models (:434-505) as
    library calls; the agent's own methods where its modules are not the library's shapes (``omegas`` not an
    nn.Linear(T d, d) with bias, a w_approx without bias, tensors off the engine's device, a φ net the setups
    refuse).  The ε draw is the reference's: random.random(), then random.randrange, from Python's random."""
    own_action, own_update = cls.get_test_action, cls.update_target_models
    if getattr(own_action, "__sfx_bound__", False):
        return

    @functools.wraps(own_action)
    def get_test_action(self, s_enc, w):
        if not self.sf.tsf_phi_test_supported(self, w):
            _fallback(self, "sync_tsf_phi_modules")
            return own_action(self, s_enc, w)
        with torch.no_grad():
            if random.random() <= self.test_epsilon:
                return torch.tensor(random.randrange(self.n_actions)).to(self.device)
            return self.sf.tsf_phi_test_action(self, s_enc, w)

    @functools.wraps(own_update)
    def update_target_models(self, w_approx, target_loss_coefficient, r, s_enc, a, s1_enc):
        if not self.sf.tsf_phi_test_supported(self, w_approx, target_loss_coefficient):
            _fallback(self, "sync_tsf_phi_modules")
            return own_update(self, w_approx, target_loss_coefficient, r, s_enc, a, s1_enc)
        return self.sf.tsf_phi_test_update(self, w_approx, target_loss_coefficient, r, s_enc, a, s1_enc)

    get_test_action.__sfx_bound__ = update_target_models.__sfx_bound__ = True
    cls.get_test_action, cls.update_target_models = get_test_action, update_target_models


def bind_phi_test(cls) -> None:
    """SFDQN_PHI.update_test_reward_mapper (agents/sfdqn_phi.py:263-305) as one library call; the agent's own
    method where w_approx is not an nn.Linear(d, 1) with bias on the engine's device or the setups refuse the
    φ net.  get_test_action already goes through GPI_w."""
    own = cls.update_test_reward_mapper
    if getattr(own, "__sfx_bound__", False):
        return

    @functools.wraps(own)
    def update_test_reward_mapper(self, w_approx, r, s_enc, a, s1_enc):
        phi_model = self.phi[0][0]
        if not self.sf.phi_test_supported(phi_model, w_approx):
            _fallback(self, "sync_phi_module")
            return own(self, w_approx, r, s_enc, a, s1_enc)
        return self.sf.phi_test_update(phi_model, w_approx, r, s_enc, a, s1_enc)

    update_test_reward_mapper.__sfx_bound__ = True
    cls.update_test_reward_mapper = update_test_reward_mapper


def lib_pre_train(self, train_tasks, n_samples_pre_train, n_cycles=5):
    """SFDQN.pre_train (sfdqn_phi.py:800-873) / TSFDQN.pre_train (tsfdqn_phi.py:1036-1109): the same loop and
    RNG draws, every minibatch update one library call; ``self.learnt_phi`` becomes the frozen net on the device
    (sfx.pretrain.LearntPhi, callable as PhiFunction.forward is).  Returns the losses as a list of floats."""
    from .. import pretrain

    self.learnt_phi, losses = pretrain.pre_train(train_tasks, n_samples_pre_train, n_cycles)
    self.learnt_phi.set_eval()
    return losses


lib_pre_train.__sfx_bound__ = True


def patch(name: str, module) -> None:
    """Bind the user's freshly loaded module ``name`` to sfx (see the module docstring)."""
    if name == "sfdqn":
        module.DeepSF = SingleFileDeepSF
    elif name in ("tsfdqn", "tsfdqn_nf"):
        module.DeepTSF = SingleFileDeepTSF
        patch_tsf_agent(module.TSFDQN)
    elif name == "agents.tsfdqn_sequential":
        patch_tsf_agent(module.TSFDQN)
    elif name == "agents.sfdqn_phi":
        m = getattr(module.SFDQN_PHI, "test_agent", None)
        if m is not None and not getattr(m, "__sfx_bound__", False):
            module.SFDQN_PHI.test_agent = _phi_synced(m)
        if hasattr(module.SFDQN_PHI, "update_test_reward_mapper"):
            bind_phi_test(module.SFDQN_PHI)
    elif name in ("sfdqn_phi", "tsfdqn_phi"):
        cls = getattr(module, "SFDQN" if name == "sfdqn_phi" else "TSFDQN", None)
        if cls is not None and hasattr(cls, "pre_train"):
            cls.pre_train = lib_pre_train
        if name == "sfdqn_phi":
            module.DeepSF = SingleFileDeepSFPhi
        else:
            module.DeepTSF = SingleFileDeepTSFPhi
            if cls is not None:
                patch_tsf_agent(cls, tsf_phi_update_test_reward_mapper)
    elif name == "agents.tsfdqn_phi":
        cls = getattr(module, "TSFDQN_PHI", None)
        if cls is None:  # not the reference's module: nothing to bind
            return
        cls.update_deep_models = tsf_phi_update_deep_models
        m = getattr(cls, "test_agent", None)
        if m is not None and not getattr(m, "__sfx_bound__", False):
            cls.test_agent = _tsf_phi_synced(m)
        if hasattr(cls, "get_test_action") and hasattr(cls, "update_target_models"):
            bind_tsf_phi_test(cls)
