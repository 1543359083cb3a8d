"""The TSF agent's test phase three ways, alternated in one process (writes profiles/native_tsf_test_phase.json):

  A  NativeEnvLoop.tsf_test_phase over the runner's built-in synthetic test tasks (no Python in the loop);
  B  NativeEnvLoop.tsf_test_phase over a Python env object (set_test_env): E callbacks per lockstep step;
  C  sfx.lockstep.test_tasks_lockstep_tsf via tools/tsf_test_phase.py: the Python lockstep path -- two
     sfx_tsf_test_actions launch sets and one sfx_tsf_test_updates launch set, a dozen small tensor
     constructions and three host round trips per lockstep step.

Shape Hopper TSF (n_s = 11, A = 27, d = 50, T = 16 heads, H = 256, G = 100; K = 0 and K = 100 planar layers),
E = 8 test tasks, horizon 500.  B's and C's tasks do the same numpy work per transition (tools/test_phase.ActionEnv's
dynamics; C's also makes the device tensors the reference's tasks return).  Protocol per K: one warm-up phase
each (graph captures), then windows of one phase each in the order A, B, C, A, B, C, ...; per path the median
and the spread (min, max) of test env-steps/s, and the host-clock µs per lockstep step (a phase's wall time /
its lockstep steps).  The test tasks' optimizer state carries over from window to window, as in a real run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-successor-features-for-transfer_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_S, A, D, T, H, G = 11, 27, 50, 16, 256, 100
# tools/tsf_test_phase.TsfEvalAgent's hyperparameters (leg C)
HP = dict(gamma=0.9, beta=0.5, lasso=0.05, lr_w=1e-3, wd_w=1e-4, lr_omega=5e-3, wd_omega=1e-5, lr_omega_decay=0.01)


class NumpyTasks:
    """E test tasks with tools/test_phase.ActionEnv's dynamics, as a set_test_env object (numpy in, numpy out)."""

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
        f = np.tanh(t.P @ t.s)
        return t.s, f, float(f @ t.w), False


def measure(K, E, hz, windows):
    from sfx.runner import NativeEnvLoop
    from tools import tsf_test_phase

    def native(env):
        eng = tsf_test_phase.make_engine(T, N_S, H, A, D, G, K, max_batch=32, seed=3)
        loop = NativeEnvLoop(eng, batch=32, capacity=1000, episode_len=hz, seed=3, schedule="tsf")
        if env is not None:
            loop.set_test_env(env)
        W = torch.empty(E, D).uniform_(-0.01, 0.01).to(eng.device)
        om = torch.rand(E, T)
        Om = (om / om.sum(dim=1, keepdim=True)).to(eng.device)
        M = torch.zeros(E, 2 * (D + T), device=eng.device)
        opt = np.zeros(E, np.int64)
        return eng, loop, (lambda: loop.tsf_test_phase(W, Om, M, opt, HP, horizon=hz, test_epsilon=0.03))

    eng_a, loop_a, run_a = native(None)
    eng_b, loop_b, run_b = native(NumpyTasks(E))
    # total_training_steps not a multiple of 1000: the reference's diagnostic prints stay off
    sf, agent, tasks = tsf_test_phase.make(E=E, T_heads=T, n_s=N_S, H=H, A=A, d=D, G=G, K=K, ep_len=hz,
                                           total_training_steps=1)
    paths = {"A": run_a, "B": run_b, "C": lambda: tsf_test_phase.run_phase(agent, tasks, True)}
    for f in paths.values():  # warm-up: graph captures, allocations
        f()
    torch.cuda.synchronize()
    secs = {k: [] for k in paths}
    for _ in range(windows):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    n = E * hz
    res = {"K": K}
    for k, v in secs.items():
        rate = [n / s for s in v]
        res[k] = {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
                  "us_per_lockstep_step": round(1e6 * statistics.median(v) / hz, 2)}
    res["A_over_C"] = round(res["A"]["median"] / res["C"]["median"], 3)
    res["B_over_C"] = round(res["B"]["median"] / res["C"]["median"], 3)
    res["A_and_B_ranges_above_C"] = min(res["A"]["min"], res["B"]["min"]) > res["C"]["max"]
    res["graphs_A"] = eng_a.graph_stats()
    loop_a.close(), loop_b.close(), eng_a.close(), eng_b.close(), sf._eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--K", type=int, nargs="*", default=[0, 100])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_tsf_test_phase.json"))
    args = ap.parse_args()
    res = {"shape": {"n_s": N_S, "A": A, "d": D, "T": T, "H": H, "G": G, "E": args.E, "horizon": args.horizon},
           "windows": args.windows, "unit": "test env-steps/s", "dtype": "fp32",
           "runs": [measure(K, args.E, args.horizon, args.windows) for K in args.K]}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
