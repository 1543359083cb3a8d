"""The learned-φ SF agent's test phase three ways, alternated in one process (writes
profiles/native_phi_test_phase.json):

  A  NativeEnvLoop.phi_test_phase over the runner's built-in synthetic test tasks (no Python in the loop);
  B  NativeEnvLoop.phi_test_phase over a Python env object (set_test_env): E callbacks per lockstep step;
  C  sfx.lockstep.test_tasks_lockstep_phi: the Python lockstep path -- one sfx_phi_test_actions launch set, a
     device read of the E actions, a dozen small tensor constructions and one sfx_phi_test_updates launch set
     per lockstep step.

Shapes: reacher_phi.cfg's (n_s = 6, A = 9, d = 12, T = 6 heads of 256 x 2, φ net 13 -> 26 x4 -> 12: the
one-workgroup kernels) and the same with the wide φ net (13 -> 2048 x4 -> 12: the E-row GEMV kernels), E = 8 test
tasks, horizon 500.  B's and C's tasks do the same numpy work per transition (tools/test_phase.ActionEnv's
dynamics; C's also makes the device tensors the reference's tasks return).  Protocol per shape: one warm-up phase
each (graph captures), then windows of one phase each in the order A, B, C, A, B, C, ...; per path the median and
the spread (min, max) of test env-steps/s, and the host-clock µs per lockstep step (a phase's wall time / its
lockstep steps).  The reward models carry over from window to window, as in a real run.  Graphs captured per leg,
and the captures after the warm-up, which must be none.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-successor-features-for-transfer_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_S, A, D, T, H = 6, 9, 12, 6, 256
N_IN = 2 * N_S + 1
NETS = {"reacher_phi": (2 * N_IN, 3), "wide": (2048, 3)}  # name -> (hid, n_mid)


class NumpyTasks:
    """E test tasks with tools/test_phase.ActionEnv's dynamics, as a set_test_env object (numpy in, numpy out; no
    φ: the phase computes it)."""

    def __init__(self, E):
        from tools.test_phase import ActionEnv

        self.t = [ActionEnv(N_S, A, D, 200 + e, "cpu") for e in range(E)]

    def reset(self, e):
        t = self.t[e]
        t.s = t.rng.standard_normal(N_S).astype(np.float32)
        return t.s

    def step(self, e, a):
        t = self.t[e]
        t.s = (np.tanh(t.M[a] @ t.s) + 0.1 * t.rng.standard_normal(N_S)).astype(np.float32)
        return t.s, None, float(np.tanh(t.P @ t.s) @ t.w), False


def phi_model(hid, n_mid, device):
    """features/deep_phi.py's φ net: Linear(n_in, hid), n_mid x Linear(hid, hid), Linear(hid, d), ReLU between."""
    dims = [N_IN] + [hid] * (n_mid + 1) + [D]
    layers = []
    for j in range(len(dims) - 1):
        layers += [torch.nn.Linear(dims[j], dims[j + 1])] + ([torch.nn.ReLU()] if j < len(dims) - 2 else [])
    return torch.nn.Sequential(*layers).to(device)


class _Log:
    def log_target_error_progress(self, d):
        pass


class PhiEvalAgent:
    """The SFDQN_PHI members sfx.lockstep.test_tasks_lockstep_phi reads (agents/sfdqn_phi.py:223-261), over the
    drop-in DeepSF_PHI."""

    def __init__(self, sf, pm, n_actions, T_ep, test_tasks, test_epsilon, device):
        self.sf, self.n_actions, self.T, self.test_epsilon, self.device = sf, n_actions, T_ep, test_epsilon, device
        self.phi = ((pm, torch.nn.MSELoss(), None), (None, None, None))
        self.encoding = lambda s: s
        self.logger = _Log()
        self.test_tasks_weights = [torch.nn.Linear(D, 1).to(device) for _ in test_tasks]

    def test_agent(self, task, test_index):
        raise AssertionError("the lockstep path runs: the tasks' episodes never end")

    def get_target_reward_mapper_error(self, r, loss, task_index, ts):
        return {"task": task_index, "reward": r, "steps": ts, "w_error": loss}


def measure(name, E, hz, windows):
    from sfx.dropin.features.deep import _flat
    from sfx.dropin.features.deep_phi import DeepSF_PHI
    from sfx.engine import SFEngine
    from sfx.init import reference_heads
    from sfx.lockstep import test_tasks_lockstep_phi
    from sfx.runner import NativeEnvLoop
    from tools.dropin_loop import psi_model_lambda
    from tools.test_phase import ActionEnv

    hid, n_mid = NETS[name]
    device = torch.device("cuda", 0)
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    pm = phi_model(hid, n_mid, device)

    def native(env):
        online, w = reference_heads(T, N_S, H, A, D, ("relu", "relu"), seed=3)
        eng = SFEngine(T, N_S, H, A, D, ("relu", "relu"), max_batch=32)
        eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
        for t in range(T):
            eng.load_head(t, online[t], 0)
            eng.load_head(t, online[t], 1)
            eng.load_w(t, w[t])
        if hid == 2 * N_IN:
            eng.phi_setup(2, n_mid, 1e-3)
        else:
            eng.phi_setup_dims(hid, n_mid, 1e-3)
        eng.phi_load(_flat(pm))
        wb, lam = torch.zeros(T, device=eng.device), torch.ones(T, device=eng.device)
        loop = NativeEnvLoop(eng, batch=32, capacity=1000, episode_len=hz, seed=3, schedule="phi", phi_bias=wb,
                             phi_lambda=lam)
        if env is not None:
            loop.set_test_env(env)
        W = torch.empty(E, D).uniform_(-0.01, 0.01).to(eng.device)
        Wb = torch.zeros(E, device=eng.device)
        return eng, loop, (lambda: loop.phi_test_phase(W, Wb, horizon=hz, test_epsilon=0.03))

    eng_a, loop_a, run_a = native(None)
    eng_b, loop_b, run_b = native(NumpyTasks(E))
    sf = DeepSF_PHI(pytorch_model_handle=psi_model_lambda(H, ("relu", "relu"), 1e-3, device), hyperparameters={},
                    target_update_ev=1000, max_batch=32)
    sf.reset()
    for t in range(T):
        sf.add_training_task(ActionEnv(N_S, A, D, 100 + t, device))
    tasks = [ActionEnv(N_S, A, D, 200 + e, device) for e in range(E)]
    agent = PhiEvalAgent(sf, pm, A, hz, tasks, 0.03, device)
    paths = {"A": run_a, "B": run_b, "C": lambda: test_tasks_lockstep_phi(agent, tasks)}
    for f in paths.values():  # warm-up: graph captures, allocations
        f()
    torch.cuda.synchronize()
    engines = {"A": eng_a, "B": eng_b, "C": sf._eng}
    warm = {k: e.graph_stats() for k, e in engines.items()}
    secs = {k: [] for k in paths}
    for _ in range(windows):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    n = E * hz
    res = {"net": name, "hid": hid, "n_mid": n_mid}
    for k, v in secs.items():
        rate = [n / s for s in v]
        res[k] = {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
                  "us_per_lockstep_step": round(1e6 * statistics.median(v) / hz, 2)}
    res["A_over_C"] = round(res["A"]["median"] / res["C"]["median"], 3)
    res["B_over_C"] = round(res["B"]["median"] / res["C"]["median"], 3)
    res["A_range_above_C"] = res["A"]["min"] > res["C"]["max"]
    res["B_range_above_C"] = res["B"]["min"] > res["C"]["max"]
    res["graphs"] = {k: e.graph_stats() for k, e in engines.items()}
    res["captures_after_warmup"] = {k: res["graphs"][k]["captures"] - warm[k]["captures"] for k in engines}
    assert res["captures_after_warmup"]["A"] == 0 and res["captures_after_warmup"]["B"] == 0, res
    loop_a.close(), loop_b.close(), eng_a.close(), eng_b.close(), sf._close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--nets", nargs="*", default=list(NETS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_phi_test_phase.json"))
    args = ap.parse_args()
    res = {"shape": {"n_s": N_S, "A": A, "d": D, "T": T, "H": H, "E": args.E, "horizon": args.horizon},
           "windows": args.windows, "unit": "test env-steps/s", "dtype": "fp32",
           "runs": [measure(name, args.E, args.horizon, args.windows) for name in args.nets]}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
