"""A test phase three ways, alternated in one process, for the SF, the TSF and the learned-φ SF agent
(``--kind sf|tsf|phi``; writes profiles/native_test_phase.json, native_tsf_test_phase.json, native_phi_test_phase.json):

  A  NativeEnvLoop.test_phase / tsf_test_phase / phi_test_phase over the runner's built-in synthetic test tasks (no
     Python in the loop);
  B  the same over a Python env object (set_test_env): E callbacks per lockstep step;
  C  the Python lockstep path, sfx.lockstep.test_tasks_lockstep / _tsf / _phi (the first two via tools/test_phase.py
     and tools/tsf_test_phase.py): per lockstep step its launch sets (sf: sfx_test_actions, sfx_test_reward_updates;
     tsf: sfx_tsf_test_actions twice, sfx_tsf_test_updates; phi: sfx_phi_test_actions, sfx_phi_test_updates), a
     dozen small tensor constructions and the host round trips between them.

Shapes, all with E = 8 test tasks and horizon 500.  sf: C2 (n_s = 17, A = 7, d = 8, T = 8 heads, H = 256).  tsf: Hopper
TSF (n_s = 11, A = 27, d = 50, T = 16 heads, H = 256, G = 100), one run per ``--K`` (0 and 100 planar layers).  phi:
reacher_phi.cfg's (n_s = 6, A = 9, d = 12, T = 6 heads of 256 x 2), one run per ``--nets``: φ net 13 -> 26 x4 -> 12 (the
one-workgroup kernels) and the wide one, 13 -> 2048 x4 -> 12 (the E-row GEMV kernels).  B's and C's tasks do the same
numpy work per transition (tools/test_phase.ActionEnv's dynamics; C's also makes the device tensors the reference's
tasks return; the φ phase computes the features itself, so its B tasks return none).

Protocol per run: one warm-up phase each (graph captures, allocations), then windows of one phase each in the order A,
B, C, A, B, C, ...; per path the median and the spread (min, max) of test env-steps/s, and the host-clock µs per
lockstep step (a phase's wall time / its lockstep steps; for A, whose env is a few C++ draws, that is the device part
and its launch).  The TSF test tasks' optimizer state and the φ kind's reward models carry over from window to window,
as in a real run.  The φ kind also counts the graphs captured per leg after the warm-up, which must be none.
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

SHAPES = {"sf": dict(n_s=17, A=7, d=8, T=8, H=256),
          "tsf": dict(n_s=11, A=27, d=50, T=16, H=256, G=100),
          "phi": dict(n_s=6, A=9, d=12, T=6, H=256)}
OUT = {"sf": "native_test_phase.json", "tsf": "native_tsf_test_phase.json", "phi": "native_phi_test_phase.json"}
# tools/tsf_test_phase.TsfEvalAgent's hyperparameters (leg C)
TSF_HP = dict(gamma=0.9, beta=0.5, lasso=0.05, lr_w=1e-3, wd_w=1e-4, lr_omega=5e-3, wd_omega=1e-5, lr_omega_decay=0.01)
PHI_NETS = {"reacher_phi": (2 * 13, 3), "wide": (2048, 3)}  # name -> (hid, n_mid); 13 = 2 n_s + 1 inputs


class NumpyTasks:
    """E test tasks with tools/test_phase.ActionEnv's dynamics, as a set_test_env object (numpy in, numpy out;
    ``features=False``: None for φ, which the phase then computes)."""

    def __init__(self, E, n_s, A, d, features=True):
        from tools.test_phase import ActionEnv

        self.t, self.n_s, self.features = [ActionEnv(n_s, A, d, 200 + e, "cpu") for e in range(E)], n_s, features

    def reset(self, e):
        t = self.t[e]
        t.s = t.rng.standard_normal(self.n_s).astype(np.float32)
        return t.s

    def step(self, e, a):
        t = self.t[e]
        t.s = (np.tanh(t.M[a] @ t.s) + 0.1 * t.rng.standard_normal(self.n_s)).astype(np.float32)
        f = np.tanh(t.P @ t.s)
        return t.s, f if self.features else None, float(f @ t.w), False


def _heads_engine(n_s, A, d, T, H):
    from sfx.engine import SFEngine
    from sfx.init import reference_heads

    online, w = reference_heads(T, n_s, H, A, d, ("relu", "relu"), seed=3)
    eng = SFEngine(T, n_s, H, A, d, ("relu", "relu"), max_batch=32)
    for t in range(T):
        eng.load_head(t, online[t], 0)
        eng.load_head(t, online[t], 1)
        eng.load_w(t, w[t])
    return eng


def _native(eng, E, hz, env, phase, **loop_kw):
    """Leg A (env None) or B over ``eng``: (engine, loop, the phase as a call)."""
    from sfx.runner import NativeEnvLoop

    loop = NativeEnvLoop(eng, batch=32, capacity=1000, episode_len=hz, seed=3, **loop_kw)
    if env is not None:
        loop.set_test_env(env)
    W = torch.empty(E, eng.d).uniform_(-0.01, 0.01).to(eng.device)
    return eng, loop, phase(loop, W)


# A kind's setup(variant, E, hz) -> (the run's leading keys, leg A, leg B, leg C's (engine once warm, phase, close))

def setup_sf(_, E, hz):
    from tools import test_phase

    n_s, A, d, T, H = SHAPES["sf"].values()
    a, b = (_native(_heads_engine(n_s, A, d, T, H), E, hz, env, lambda loop, W: lambda: loop.test_phase(W, horizon=hz))
            for env in (None, NumpyTasks(E, n_s, A, d)))
    sf, agent, tasks = test_phase.make(E=E, T_heads=T, n_s=n_s, H=H, A=A, d=d, ep_len=hz, device_mapper=True)
    return {}, a, b, (lambda: sf._eng, lambda: test_phase.run_phase(agent, tasks, True), sf._close)


def setup_tsf(K, E, hz):
    from tools import tsf_test_phase

    n_s, A, d, T, H, G = SHAPES["tsf"].values()

    def phase(loop, W):
        om = torch.rand(E, T)
        Om = (om / om.sum(dim=1, keepdim=True)).to(W.device)
        M, opt = torch.zeros(E, 2 * (d + T), device=W.device), np.zeros(E, np.int64)
        return lambda: loop.tsf_test_phase(W, Om, M, opt, TSF_HP, horizon=hz, test_epsilon=0.03)

    a, b = (_native(tsf_test_phase.make_engine(T, n_s, H, A, d, G, K, max_batch=32, seed=3), E, hz, env, phase,
                    schedule="tsf") for env in (None, NumpyTasks(E, n_s, A, d)))
    # total_training_steps not a multiple of 1000: the reference's diagnostic prints stay off
    sf, agent, tasks = tsf_test_phase.make(E=E, T_heads=T, n_s=n_s, H=H, A=A, d=d, G=G, K=K, ep_len=hz,
                                           total_training_steps=1)
    return {"K": K}, a, b, (lambda: sf._eng, lambda: tsf_test_phase.run_phase(agent, tasks, True), sf._eng.close)


class _NoLog:
    def log_target_error_progress(self, d):
        pass


class PhiEvalAgent:
    """The SFDQN_PHI members sfx.lockstep.test_tasks_lockstep_phi reads (agents/sfdqn_phi.py:223-261), over the
    drop-in DeepSF_PHI."""

    def __init__(self, sf, pm, n_actions, T_ep, test_tasks, test_epsilon, device):
        self.sf, self.n_actions, self.T, self.test_epsilon, self.device = sf, n_actions, T_ep, test_epsilon, device
        self.phi = ((pm, torch.nn.MSELoss(), None), (None, None, None))
        self.encoding = lambda s: s
        self.logger = _NoLog()
        self.test_tasks_weights = [torch.nn.Linear(SHAPES["phi"]["d"], 1).to(device) for _ in test_tasks]

    def test_agent(self, task, test_index):
        raise AssertionError("the lockstep path runs: the tasks' episodes never end")

    def get_target_reward_mapper_error(self, r, loss, task_index, ts):
        return {"task": task_index, "reward": r, "steps": ts, "w_error": loss}


def setup_phi(name, E, hz):
    from sfx.dropin.features.deep import _flat
    from sfx.dropin.features.deep_phi import DeepSF_PHI
    from sfx.lockstep import test_tasks_lockstep_phi
    from tools.dropin_loop import psi_model_lambda
    from tools.test_phase import ActionEnv

    n_s, A, d, T, H = SHAPES["phi"].values()
    hid, n_mid = PHI_NETS[name]
    device = torch.device("cuda", 0)
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    # features/deep_phi.py's φ net: Linear(n_in, hid), n_mid x Linear(hid, hid), Linear(hid, d), ReLU between
    dims = [2 * n_s + 1] + [hid] * (n_mid + 1) + [d]
    layers = []
    for j in range(len(dims) - 1):
        layers += [torch.nn.Linear(dims[j], dims[j + 1])] + ([torch.nn.ReLU()] if j < len(dims) - 2 else [])
    pm = torch.nn.Sequential(*layers).to(device)

    def native(env):
        eng = _heads_engine(n_s, A, d, T, H)
        eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
        if hid == 2 * (2 * n_s + 1):
            eng.phi_setup(2, n_mid, 1e-3)
        else:
            eng.phi_setup_dims(hid, n_mid, 1e-3)
        eng.phi_load(_flat(pm))
        Wb = torch.zeros(E, device=eng.device)
        return _native(eng, E, hz, env, lambda loop, W: lambda: loop.phi_test_phase(W, Wb, horizon=hz, test_epsilon=0.03),
                       schedule="phi", phi_bias=torch.zeros(T, device=eng.device),
                       phi_lambda=torch.ones(T, device=eng.device))

    a, b = native(None), native(NumpyTasks(E, n_s, A, d, features=False))
    sf = DeepSF_PHI(pytorch_model_handle=psi_model_lambda(H, ("relu", "relu"), 1e-3, device), hyperparameters={},
                    target_update_ev=1000, max_batch=32)
    sf.reset()
    for t in range(T):
        sf.add_training_task(ActionEnv(n_s, A, d, 100 + t, device))
    tasks = [ActionEnv(n_s, A, d, 200 + e, device) for e in range(E)]
    agent = PhiEvalAgent(sf, pm, A, hz, tasks, 0.03, device)
    run_c = lambda: test_tasks_lockstep_phi(agent, tasks)  # noqa: E731
    return {"net": name, "hid": hid, "n_mid": n_mid}, a, b, (lambda: sf._eng, run_c, sf._close)


def measure(kind, variant, E, hz, windows):
    head, (eng_a, loop_a, run_a), (eng_b, loop_b, run_b), (eng_c, run_c, close_c) = SETUP[kind](variant, E, hz)
    paths = {"A": run_a, "B": run_b, "C": run_c}
    for f in paths.values():  # warm-up: graph captures, allocations
        f()
    torch.cuda.synchronize()
    engines = {"A": eng_a, "B": eng_b, "C": eng_c()}  # the drop-in makes C's engine on first use
    warm = {k: e.graph_stats() for k, e in engines.items()}
    secs = {k: [] for k in paths}
    for _ in range(windows):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    res = dict(head, **summary(secs, E * hz, hz))
    graphs = {k: e.graph_stats() for k, e in engines.items()}
    if kind == "phi":
        res["A_range_above_C"] = res["A"]["min"] > res["C"]["max"]
        res["B_range_above_C"] = res["B"]["min"] > res["C"]["max"]
        res["graphs"] = graphs
        res["captures_after_warmup"] = {k: graphs[k]["captures"] - warm[k]["captures"] for k in engines}
        assert res["captures_after_warmup"]["A"] == 0 and res["captures_after_warmup"]["B"] == 0, res
    else:
        if kind == "tsf":
            res["A_and_B_ranges_above_C"] = min(res["A"]["min"], res["B"]["min"]) > res["C"]["max"]
        res["graphs_A"] = graphs["A"]
    loop_a.close(), loop_b.close(), eng_a.close(), eng_b.close(), close_c()
    return res


def summary(secs, n, hz):
    """Per path the median, min and max rate of its windows and the µs per lockstep step; A and B over C."""
    res = {}
    for k, v in secs.items():
        rate = [n / s for s in v]
        res[k] = {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
                  "us_per_lockstep_step": round(1e6 * statistics.median(v) / hz, 2)}
    res["A_over_C"] = round(res["A"]["median"] / res["C"]["median"], 3)
    res["B_over_C"] = round(res["B"]["median"] / res["C"]["median"], 3)
    return res


SETUP = {"sf": setup_sf, "tsf": setup_tsf, "phi": setup_phi}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=list(SETUP), default="sf")
    ap.add_argument("--E", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=500)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--K", type=int, nargs="*", default=[0, 100], help="tsf: planar layers, one run each")
    ap.add_argument("--nets", nargs="*", default=list(PHI_NETS), help="phi: φ nets, one run each")
    ap.add_argument("--out", default=None, help="default: the kind's file under profiles/")
    args = ap.parse_args()
    variants = {"sf": [None], "tsf": args.K, "phi": args.nets}[args.kind]
    runs = [measure(args.kind, v, args.E, args.horizon, args.windows) for v in variants]
    res = {"shape": dict(SHAPES[args.kind], E=args.E, horizon=args.horizon), "windows": args.windows,
           "unit": "test env-steps/s", "dtype": "fp32"}
    if args.kind == "sf":
        res.update(runs[0])
    else:
        res["runs"] = runs
    with open(args.out or os.path.join(ROOT, "profiles", OUT[args.kind]), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()


