"""The seed recipe behind tests/golden/calls_sfdqn_phi_singlefile.npz and calls_tsfdqn_phi_singlefile.npz (our own
code, data generation only): the single-file learned-φ agents sfdqn_phi.py / tsfdqn_phi.py on synthetic tasks -- a
short pre_train, then a short main phase over 2 tasks at the shapes of tests/golden/recipe.py's single-file recipes
(n_s 17, H 32, A 7, d 8, batches of 8).  24 samples a task with a target sync every 5 updates give three syncs per
head and, on the second task, GPI over both heads; one test phase per task (10 episodes, each ended by the test task
after 4 steps).

tools/gen_phi_singlefile_golden.py runs it with the real reference; tests/test_gpu_dropin_phi_singlefile.py builds
sfx's bound classes from the same hyper-parameters and replays the log.
"""
from __future__ import annotations

import torch

from tests.golden.recipe import AGENT_RUN_SEQ, AGENT_RUN_TSF, AgentTask, agent_psi_lambda

PRE = dict(n=20, cycles=2)     # pre_train(train_tasks, n, cycles): 2 * 2 * 20 transitions, 49 updates of batch 32
AGENT_RUN_SEQ_PHI = dict(AGENT_RUN_SEQ, seed=21, T_tasks=2, n_samples=24, n_test_ev=24)
AGENT_RUN_TSF_PHI = dict(AGENT_RUN_TSF, seed=23, T_tasks=2, n_samples=24, n_test_ev=24)


class PhiAgentTask(AgentTask):
    """tasks/hopper_phi.py's interface on the synthetic task: the action is one input column of the φ net, there are
    no true reward weights (get_w raises, as the reference's does), and `features` is never the source of φ."""

    def action_dim(self):
        return 1

    def get_w(self):
        raise NotImplementedError("a learned-φ task has no true reward weights")

    def features(self, state, action, next_state):
        raise AssertionError("the learned-φ agents take φ from the pre-trained net")


def _seed(c):
    import random

    import numpy as np

    random.seed(c["seed"])
    np.random.seed(c["seed"])
    torch.manual_seed(c["seed"])


def _tasks(c, device, base):
    tasks = [PhiAgentTask(c["n_s"], c["A"], c["d"], i, base + i, device, c["task_terminal_every"], tensor_reward=True)
             for i in range(c["T_tasks"])]
    # the test task ends its episodes after 4 steps: test_agent's 10 episodes stay short, and so do the fixtures
    return tasks, [PhiAgentTask(c["n_s"], c["A"], c["d"], c["T_tasks"], base + 100, device, 4, tensor_reward=True)]


def agent_run_sequential_phi(DeepSF, SFDQN, ReplayBuffer, device, pretrained=lambda agent: None):
    """sfdqn_phi.py's __main__ in small: build, pre_train, train.  `pretrained(agent)` runs between the two phases
    (the generator logs the frozen net there).  Returns (agent, tasks, test_tasks, returns)."""
    c = AGENT_RUN_SEQ_PHI
    _seed(c)
    tasks, test_tasks = _tasks(c, device, 700)
    sf = DeepSF(pytorch_model_handle=agent_psi_lambda(c["H"], c["acts"], c["lr"], device),
                target_update_ev=c["target_update_ev"], hyperparameters=c["hp"])
    agent = SFDQN(deep_sf=sf, buffer_handle=lambda: ReplayBuffer(**c["buffer"]), gamma=c["gamma"], T=c["episode_T"],
                  encoding="task", epsilon=c["epsilon"], use_gpi=True, test_epsilon=0.03, hyperparameters=c["hp"])
    agent.pre_train(tasks, PRE["n"], PRE["cycles"])
    pretrained(agent)
    returns = agent.train(tasks, c["n_samples"], test_tasks=test_tasks, n_test_ev=c["n_test_ev"])
    return agent, tasks, test_tasks, returns


def agent_run_tsf_phi(DeepTSF, TSFDQN, ReplayBuffer, device, pretrained=lambda agent: None):
    """tsfdqn_phi.py's __main__ in small; see agent_run_sequential_phi."""
    c = AGENT_RUN_TSF_PHI
    _seed(c)
    tasks, test_tasks = _tasks(c, device, 900)
    sf = DeepTSF(pytorch_model_handle=agent_psi_lambda(c["H"], c["acts"], c["lr"], device), use_true_reward=False,
                 target_update_ev=c["target_update_ev"], hyperparameters=c["hp"])
    agent = TSFDQN(deep_sf=sf, buffer_handle=lambda: ReplayBuffer(**c["buffer"]), gamma=c["gamma"], T=c["episode_T"],
                   encoding="task", epsilon=c["epsilon"], use_gpi=True, test_epsilon=0.03, hyperparameters=c["hp"])
    agent.pre_train(tasks, PRE["n"], PRE["cycles"])
    pretrained(agent)
    returns = agent.train(tasks, c["n_samples"], test_tasks=test_tasks, n_test_ev=c["n_test_ev"])
    return agent, tasks, test_tasks, returns
