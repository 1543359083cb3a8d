#!/usr/bin/env python3
"""Timing of the frozen featurizer of the single-file learned-φ agents' main phase -> profiles/frozen_phi_runner.json.

Shapes: the reference's -- PhiFunction 9 -> 128 -> 256 -> 12 (n_s 4, d 12; sfdqn_phi.py:90-123), ψ heads of width 256
with 2 hidden layers, 9 actions, minibatches of 32, 4 tasks (TSF: g_i = Linear(4, 16), h = Linear(16, 12)).

  1. the featurizer alone: µs per sfx_pre_features_rows (k_pre_rows: one workgroup per 16-row tile, activations in
     LDS) beside sfx_pre_features (k_pre_fwd: one workgroup, activations in global scratch) at 32 rows and at 1 row;
     windows of CALLS calls alternated between the four, a host clock around calls that end in one synchronise and a
     pair of device events next to it;
  2. what the featurizer launch costs in the native runner: env-steps/s of NativeEnvLoop(schedule="active" | "tsf")
     with the featurizer and without it (φ from the env: the existing path of the same build), windows of STEPS
     steps alternated between the four loops;
  3. the main-phase step driven from Python, what a user of the drop-in gets: LearntPhi on one row, then the update
     on a device-resident minibatch, then the select with one host read of the action (no env, no replay);
  4. the same step in the native runner with the featurizer (item 2's figure) and its ratio to item 3.

--trace runs only item 1's four calls, a few hundred times each, for a `rocprofv3 --kernel-trace --stats` run of its
own (where the time goes); nothing is timed then.  A missing GPU is an error.

Usage:  python tools/frozen_phi_runner_bench.py [--windows 15] [--calls 200] [--steps 600] [--out profiles/frozen_phi_runner.json]
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/frozen_phi_runner_bench.py --trace
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "deep-successor-features-for-transfer_amd"))

import torch  # noqa: E402

N_S, D, HIDDEN, A, B, T, H, G = 4, 12, (128, 256), 9, 32, 4, 256, 16
TASK = 1


def summary(host, device=None):
    out = dict(median=statistics.median(host), min=min(host), max=max(host), windows=len(host))
    if device:
        out["device_median"] = statistics.median(device)
    return out


def call_windows(fns, n_windows, calls, warm=3):
    """µs per call: the variants' windows interleaved (a, b, c, d, a, ...) after `warm` windows of each."""
    res = {k: ([], []) for k in fns}
    for w in range(warm + n_windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if w >= warm:
                res[k][0].append((time.perf_counter() - t0) / calls * 1e6)
                res[k][1].append(e0.elapsed_time(e1) / calls * 1e3)
    return {k: dict(summary(h, d), unit="us per call", calls=calls) for k, (h, d) in res.items()}


def psi_engine(tsf):
    from sfx.engine import SFEngine
    from sfx.init import reference_heads

    acts = ("relu", "relu")
    online, w = reference_heads(T, N_S, H, A, D, acts, seed=0)
    eng = SFEngine(T, N_S, H, A, D, acts, max_batch=B)
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    eng.set_target_update_ev(1000)
    for t in range(T):
        eng.load_head(t, online[t], 0)
        eng.load_head(t, online[t], 1)
        eng.load_w(t, w[t])
    if tsf:
        gen = torch.Generator().manual_seed(4)
        eng.tsf_setup(G, 0, 1.0, 1e-3, 0.0, 1e-3, 0.0)
        for t in range(T):
            eng.tsf_load_g(t, torch.empty(G * N_S + G).uniform_(-0.3, 0.3, generator=gen))
        eng.tsf_load_h(torch.empty(D * G + D).uniform_(-0.2, 0.2, generator=gen))
    return eng


def pre_engine(dev):
    from sfx import pretrain
    from tests import pretrain_ref as PR

    eng = pretrain.PreEngine(N_S, D, T, HIDDEN, max_batch=B, device=dev)
    eng.load(PR.problem(N_S, D, T, HIDDEN, 1).flat)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=600, help="env steps per runner window")
    ap.add_argument("--trace", action="store_true", help="only item 1's calls, for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_phi_runner.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_phi_runner_bench needs a GPU")
    from sfx._lib import lib
    from sfx.pretrain import LearntPhi
    from sfx.runner import NativeEnvLoop
    from tests import pretrain_ref as PR

    dev = torch.device("cuda:0")
    pre = pre_engine(dev)
    gen = torch.Generator().manual_seed(2)
    S, a, r, S1 = (x.to(dev) for x in PR.batch(N_S, A, B, gen))
    phi_rows, phi_fwd = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
    pre._bind_stream()
    h, ptrs = pre.handle, (S.data_ptr(), a.data_ptr(), S1.data_ptr())
    calls = {f"sfx_pre_features_rows_M{m}": (lambda m=m: lib.sfx_pre_features_rows(h, *ptrs, m, phi_rows.data_ptr()))
             for m in (B, 1)}
    calls.update({f"sfx_pre_features_B{m}": (lambda m=m: lib.sfx_pre_features(h, *ptrs, m, phi_fwd.data_ptr()))
                  for m in (B, 1)})
    # same outputs first: the two kernels agree bit for bit before anything is timed
    for m in (B, 1):
        assert calls[f"sfx_pre_features_rows_M{m}"]() == 0 and calls[f"sfx_pre_features_B{m}"]() == 0
        torch.cuda.synchronize()
        assert torch.equal(phi_rows[:m], phi_fwd[:m]), f"{m} rows: the two forwards differ"
    if args.trace:
        for fn in calls.values():
            for _ in range(300):
                fn()
            torch.cuda.synchronize()
        return
    assert args.windows >= 15
    res = {"shape": dict(n_s=N_S, d=D, phi_hidden=list(HIDDEN), H=H, A=A, B=B, T=T, G=G),
           "device": torch.cuda.get_device_name(0)}
    res["featurizer"] = call_windows(calls, args.windows, args.calls)

    # 2. the runner with and without the featurizer, four loops alternated
    loops, keep = {}, []
    for schedule in ("active", "tsf"):
        for feat in (True, False):
            eng = psi_engine(schedule == "tsf")
            loop = NativeEnvLoop(eng, batch=B, capacity=100000, gamma=0.9, epsilon=0.1, episode_len=500, seed=1,
                                 schedule=schedule, featurizer=pre if feat else None)
            loop.prefill(4 * B)
            loop.set_task(TASK)
            loop.warm()
            loops[f"{schedule}_{'featurizer' if feat else 'env_phi'}"] = loop
            keep.append(eng)
    rates = {k: [] for k in loops}
    for w in range(3 + args.windows):
        for k, loop in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.run(args.steps)
            dt = time.perf_counter() - t0
            if w >= 3:
                rates[k].append(args.steps / dt)
    res["runner"] = {k: dict(summary(v), unit="env-steps/s", steps=args.steps, stats=loops[k].stats())
                     for k, v in rates.items()}
    for schedule in ("active", "tsf"):
        f, e = res["runner"][f"{schedule}_featurizer"]["median"], res["runner"][f"{schedule}_env_phi"]["median"]
        res["runner"][f"{schedule}_featurizer_cost_us_per_step"] = (1.0 / f - 1.0 / e) * 1e6
    for loop in loops.values():
        loop.close()

    # 3. the step driven from Python: LearntPhi on one row, the update, the select with one host read
    learnt = LearntPhi(pre)
    gam, rr = torch.full((B,), 0.9, device=dev), r.reshape(-1, 1).contiguous()
    PHI = pre.features(S, a, S1)
    s_row, a_row, s1_row = S[:1].contiguous(), a[0], S1[:1].contiguous()
    sel_host = torch.zeros(2, dtype=torch.long, pin_memory=True)
    py = {}
    for schedule in ("active", "tsf"):
        eng = psi_engine(schedule == "tsf")
        upd = eng.tsf_update if schedule == "tsf" else eng.update
        losses = torch.zeros(3, device=dev)

        def step(eng=eng, upd=upd, losses=losses):
            learnt(s_row, a_row, s1_row)     # the φ the agent appends to its buffer
            upd(TASK, S, a, rr, PHI, S1, gam, True, losses=losses)
            sel_host.copy_(eng.select_action(s_row, TASK, True), non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return int(sel_host[1])

        py[schedule] = step
        keep.append(eng)
    t = call_windows(py, args.windows, args.calls)
    res["python_step"] = {k: dict(v, steps_per_s=1e6 / v["median"]) for k, v in t.items()}
    for schedule in ("active", "tsf"):
        res[f"native_over_python_{schedule}"] = res["runner"][f"{schedule}_featurizer"]["median"] / \
            res["python_step"][schedule]["steps_per_s"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
