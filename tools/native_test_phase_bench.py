"""The SF agent's test phase three ways, alternated in one process (writes profiles/native_test_phase.json):

  A  NativeEnvLoop.test_phase over the runner's built-in synthetic test tasks (no Python in the loop);
  B  NativeEnvLoop.test_phase over a Python env object (set_test_env): E callbacks per lockstep step;
  C  sfx.lockstep.test_tasks_lockstep via tools/test_phase.py: the Python lockstep path -- one
     sfx_test_actions launch set, one sfx_test_reward_updates launch, E small host->device copies and a
     device read of the actions per lockstep step.

Shape C2 (n_s = 17, A = 7, d = 8, T = 8 heads, H = 256), E = 8 test tasks, horizon 500.  B's and C's tasks
do the same numpy work per transition (tools/test_phase.ActionEnv's dynamics; C's also makes the device
tensors the reference's tasks return).  Protocol: one warm-up phase each (graph captures), then windows of one
phase each in the order A, B, C, A, B, C, ...; per path the median and the spread (min, max) of test
env-steps/s, and the host-clock µs per lockstep step (a phase's wall time / its lockstep steps; for A, whose
env is a few C++ draws, that is the device part and its launch).
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

N_S, A, D, T, H = 17, 7, 8, 8, 256


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_test_phase.json"))
    args = ap.parse_args()
    E, hz = args.E, args.horizon

    from sfx.engine import SFEngine
    from sfx.init import reference_heads
    from sfx.runner import NativeEnvLoop
    from tools import test_phase

    def native(env):
        online, w = reference_heads(T, N_S, H, A, D, ("relu", "relu"), seed=3)
        eng = SFEngine(T, N_S, H, A, D, ("relu", "relu"), max_batch=32)
        for t in range(T):
            eng.load_head(t, online[t], 0)
            eng.load_head(t, online[t], 1)
            eng.load_w(t, w[t])
        loop = NativeEnvLoop(eng, batch=32, capacity=1000, episode_len=hz, seed=3)
        if env is not None:
            loop.set_test_env(env)
        W = torch.empty(E, D).uniform_(-0.01, 0.01).to(eng.device)
        return eng, loop, (lambda: loop.test_phase(W, horizon=hz))

    eng_a, loop_a, run_a = native(None)
    eng_b, loop_b, run_b = native(NumpyTasks(E))
    sf, agent, tasks = test_phase.make(E=E, T_heads=T, n_s=N_S, H=H, A=A, d=D, ep_len=hz, device_mapper=True)
    paths = {"A": run_a, "B": run_b, "C": lambda: test_phase.run_phase(agent, tasks, True)}
    for f in paths.values():  # warm-up: graph captures, allocations
        f()
    torch.cuda.synchronize()
    secs = {k: [] for k in paths}
    for _ in range(args.windows):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    n = E * hz
    res = {"shape": {"n_s": N_S, "A": A, "d": D, "T": T, "H": H, "E": E, "horizon": hz},
           "windows": args.windows, "unit": "test env-steps/s", "dtype": "fp32"}
    for k, v in secs.items():
        rate = [n / s for s in v]
        res[k] = {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
                  "us_per_lockstep_step": round(1e6 * statistics.median(v) / hz, 2)}
    res["A_over_C"] = round(res["A"]["median"] / res["C"]["median"], 3)
    res["B_over_C"] = round(res["B"]["median"] / res["C"]["median"], 3)
    res["graphs_A"] = eng_a.graph_stats()
    loop_a.close(), loop_b.close(), eng_a.close(), eng_b.close(), sf._close()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
