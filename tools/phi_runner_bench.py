#!/usr/bin/env python3
"""Env-steps/s of the learned-φ agents' training step: the native runner against the same steps driven from
Python, in one process and one build, on one GPU, in alternating windows.

Shapes:
  * sf_phi:   reacher_phi.cfg with main_sfdqn_phi_torch.py's nets: 6 train tasks, n_s = 6, A = 9, d = 12, ψ heads
              256 x 2, φ net 13 -> 26 x4 -> 12 (phi_setup(2, 3): the one-workgroup kernels), B = 32, use_gpi False,
              target sync every 1000 updates, γ 0.9, ε 0.1, episodes of 500 steps;
  * tsf_phi:  tools/tsf_phi_bench.py's: φ net 13 -> 2048 x4 -> 12 (12.6 M parameters, the MFMA kernels), T = 4,
              B = 32, use_gpi True, g_i and h plain Linears.

The two sides of a pair:
  * native:   NativeEnvLoop(schedule="phi" | "tsf_phi").run(n) on the built-in synthetic task: env, host replay ring
              and its uniform minibatch, staging, the pre-launched step graphs (everything an env step costs);
  * python:   per step eng.phi_update / eng.tsf_phi_update on a fixed device minibatch, eng.gpi for the next state,
              the bias added and the argmax taken in torch, and ONE host read of the action -- the calls of the
              drop-in agents' loop (features/deep_phi.py GPI_w, update_successor).  No env, no replay and no
              host-to-device copy on this side, so the comparison flatters it.

Windows alternate native / python (--windows pairs of --steps env steps each) after a warm-up of both, so clock and
thermal drift fall on both sides alike; reported: the median window and the spread (min, max) of each side, and
the ratio of the medians.  Writes one JSON object (--out, default profiles/phi_runner.json) and prints it.
Usage:  python tools/phi_runner_bench.py [--windows 7] [--steps 2000]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "deep-successor-features-for-transfer_amd")):
    sys.path.insert(0, os.path.abspath(p))

from tests import tsf_phi_ref as TP  # noqa: E402
from tools.tsf_phi_bench import problem  # noqa: E402

SHAPES = {
    # name: (Net, T, B, tsf, use_gpi, target_update_ev, φ setup)
    "sf_phi": (TP.Net(6, 256, 9, 12, ("relu", "relu"), 26, 3), 6, 32, False, False, 1000, ("mul", 2)),
    "tsf_phi": (TP.Net(6, 256, 9, 12, ("relu", "relu"), 2048, 3), 4, 32, True, True, 1000, ("dims", 2048)),
}


def build(name, dev):
    from sfx.engine import SFEngine
    from sfx.runner import NativeEnvLoop

    net, T, B, tsf, use_gpi, ev, (how, arg) = SHAPES[name]
    st = problem(net, T)

    def engine():
        eng = SFEngine(T, net.n_s, net.H, net.A, net.d, net.acts, max_batch=B, device="cuda:0")
        eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
        eng.set_target_update_ev(ev)
        for t in range(T):
            eng.load_head(t, st.online[t], 0)
            eng.load_head(t, st.target[t], 1)
            eng.load_w(t, st.w[t])
        if how == "mul":
            eng.phi_setup(arg, net.n_mid, 1e-3)
        else:
            eng.phi_setup_dims(arg, net.n_mid, 1e-3)
        eng.phi_load(st.phi)
        if tsf:
            eng.tsf_setup(net.d, 0)
            for t in range(T):
                eng.tsf_load_g(t, st.g[t])
            eng.tsf_load_h(st.h)
        return eng

    # native side
    e1 = engine()
    wb1, lam1 = torch.zeros(T, device=dev), torch.ones(T, device=dev)
    loop = NativeEnvLoop(e1, batch=B, capacity=100_000, gamma=0.9, epsilon=0.1, episode_len=500, use_gpi=use_gpi, seed=1,
                         schedule="tsf_phi" if tsf else "phi", upd_use_gpi=use_gpi, phi_bias=wb1, phi_lambda=lam1)
    loop.prefill(4 * B)
    loop.set_task(0)
    loop.warm()

    # python side: its own engine, fixed device inputs
    e2 = engine()
    wb2, lam2 = torch.zeros(T, device=dev), torch.ones(T, device=dev)
    gen = torch.Generator().manual_seed(3)
    s, s1 = torch.randn(B, net.n_s, generator=gen).to(dev), torch.randn(B, net.n_s, generator=gen).to(dev)
    a = torch.randint(0, net.A, (B,), generator=gen).to(dev)
    r = torch.rand(B, generator=gen).to(dev)
    gamma = torch.full((B,), 0.9).to(dev)
    snext = torch.randn(1, net.n_s, generator=gen).to(dev)
    losses = torch.empty(4, device=dev)
    upd = e2.tsf_phi_update if tsf else e2.phi_update

    def py_steps(n):
        act = 0
        for _ in range(n):
            upd(0, s, a, r, s1, gamma, wb2[0:1], lam2[0:1], use_gpi=use_gpi, losses=losses)
            _, q, _, _ = e2.gpi(snext, w_index=0)
            q = q + wb2[0]
            c = torch.argmax(torch.max(q, dim=2).values, dim=1) if use_gpi else 0
            act = int(torch.argmax(q[0, c, :].reshape(-1)))  # the step's one host read
        return act

    def close():
        loop.close()
        e1.close()
        e2.close()

    shape = dict(n_s=net.n_s, A=net.A, d=net.d, H=net.H, T=T, B=B, hid=net.hid, n_mid=net.n_mid, phi_params=net.P_phi,
                 use_gpi=use_gpi, target_update_ev=ev)
    return shape, loop, py_steps, losses, close


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(rates):
    return dict(median=round(statistics.median(rates), 1), min=round(min(rates), 1), max=round(max(rates), 1),
                windows=[round(x, 1) for x in rates])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--shapes", default="sf_phi,tsf_phi")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phi_runner.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(0), arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
               windows=args.windows, steps_per_window=args.steps, unit="env steps / s", shapes={})
    for name in args.shapes.split(","):
        shape, loop, py_steps, losses, close = build(name, dev)
        loop.run(args.warmup)
        py_steps(args.warmup)
        native, python = [], []
        for _ in range(args.windows):
            native.append(args.steps / timed(lambda: loop.run(args.steps)))
            python.append(args.steps / timed(lambda: py_steps(args.steps)))
        assert bool(torch.isfinite(losses).all()) and all(x == x for x in loop.phi_losses()), (losses, loop.phi_losses())
        stats = loop.stats()
        n, p = summary(native), summary(python)
        out["shapes"][name] = dict(shape=shape, native=n, python=p, native_over_python=round(n["median"] / p["median"], 3),
                                   native_us_per_step=round(1e6 / n["median"], 1), python_us_per_step=round(1e6 / p["median"], 1),
                                   prelaunched_share=round(stats["prelaunched"] / max(1, stats["env_steps"]), 3),
                                   retried=stats["retried"])
        close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
