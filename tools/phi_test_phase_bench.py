#!/usr/bin/env python3
"""Time one test step of the learned-φ TSF agent (agents/tsfdqn_phi.py get_test_action + update_target_models) at
the shape of main_tsfdqn_phi_torch.py: φ net 13 -> 2048 x4 -> 12 (12.6 M fp32 parameters), n_s = 6, A = 9,
d = 12, ψ heads 256 x 2, T = 4.  In one process, on one GPU:

  * library:  sfx_tsf_phi_test_action + sfx_tsf_phi_test_update per step (the action stays on the device and
              feeds the update);
  * eager:    the same step in torch eager on the same GPU (tests/phi_test_ref.py moved to the device: the ψ and
              g forwards, the φ net, autograd, a freshly built Adam's step) -- what the drop-in ran before the
              test phase moved into the library;
  * one-row φ forward alone (sfx_phi_features, B = 1: csrc/sfx_phitest.h k_phi1_fwd) with its effective
    bandwidth, φ-net bytes / time, and next to it the update's forward at B = 2 (k_phiw_fwd), the yardstick.

Neither side reads anything back inside a timed window.  A window is --window steps between two device events;
the figure is the median over --windows windows after warm-up, the spread the min and max window.  That is the
time a caller sees, launches included.  The kernels' own time comes from a separate leg with the library's
launch instrumentation on (sfx_prof_enable: start / stop timestamps of every dispatch packet): µs of kernel
time per call and the launches it took, for the two φ forwards and the library step.

Writes one JSON object (--out, default profiles/phi_test_phase.json) and prints it.
Usage:  python tools/phi_test_phase_bench.py [--windows 15] [--window 40]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "deep-successor-features-for-transfer_amd")):
    sys.path.insert(0, os.path.abspath(p))

from tests import phi_test_ref as PT  # noqa: E402
from tests import tsf_phi_ref as TP  # noqa: E402


def problem(net, T, seed=0):
    from sfx.init import reference_heads

    online, w = reference_heads(T, net.n_s, net.H, net.A, net.d, net.acts, seed=seed)
    torch.manual_seed(seed + 1)
    flat = lambda m: torch.cat([m.weight.detach().reshape(-1), m.bias.detach()])
    phi0 = torch.cat([flat(torch.nn.Linear(i, o)) for o, i in net.phi_dims])
    g = torch.stack([flat(torch.nn.Linear(net.n_s, net.d)) for _ in range(T)])
    h = flat(torch.nn.Linear(net.d, net.d))
    om, wm = torch.nn.Linear(T * net.d, net.d), torch.nn.Linear(net.d, 1)
    st = TP.State(net, online.clone(), online.clone() + 0.01, w.clone(), torch.zeros(T), phi0, g, h, torch.ones(T))
    tt = PT.TestTask(om.weight.detach().clone(), om.bias.detach().clone(),
                     torch.empty(net.d).uniform_(-0.01, 0.01), wm.bias.detach().clone(), torch.ones(1))
    return st, tt


def windows_us(fn, windows, window):
    """µs per call: `windows` windows of `window` calls, each between two device events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(windows)]
    for a, b in ev:
        a.record()
        for _ in range(window):
            fn()
        b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) / window for a, b in ev]


def stats(xs):
    return dict(median=round(statistics.median(xs), 2), min=round(min(xs), 2), max=round(max(xs), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--eager-window", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hid", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phi_test_phase.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("phi_test_phase_bench needs a GPU")
    from sfx.engine import SFEngine

    net, T, gamma = TP.Net(6, 256, 9, 12, ("relu", "relu"), args.hid, 3), 4, 0.9
    st, tt = problem(net, T)
    dev = torch.device("cuda", 0)
    eng = SFEngine(T, net.n_s, net.H, net.A, net.d, net.acts, max_batch=32, device="cuda:0")
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    for t in range(T):
        eng.load_head(t, st.online[t], 0)
        eng.load_head(t, st.target[t], 1)
        eng.load_w(t, st.w[t])
    eng.phi_setup_dims(net.hid, net.n_mid, 1e-3)
    eng.phi_load(st.phi)
    eng.tsf_setup(net.d, 0)
    for t in range(T):
        eng.tsf_load_g(t, st.g[t])
    eng.tsf_load_h(st.h)
    gen = torch.Generator().manual_seed(3)
    s, s1 = torch.randn(net.n_s, generator=gen).to(dev), torch.randn(net.n_s, generator=gen).to(dev)
    s2, s12 = torch.randn(2, net.n_s, generator=gen).to(dev), torch.randn(2, net.n_s, generator=gen).to(dev)
    a1, a2 = torch.zeros(1, dtype=torch.long, device=dev), torch.zeros(2, dtype=torch.long, device=dev)
    r = 0.5

    td = tt.to(dtype=torch.float32, device=dev)
    act, losses = torch.empty((), dtype=torch.long, device=dev), torch.empty(3, device=dev)

    def lib_step():
        eng.tsf_phi_test_action(s, td.omega_w, td.omega_b, td.w, td.wb, out=act)
        eng.tsf_phi_test_update(s, act, r, s1, gamma, td.omega_w, td.omega_b, td.w, td.wb, td.lam, losses=losses)

    sd, te = st.to(device=dev), tt.to(dtype=torch.float32, device=dev)

    def eager_step():
        a = torch.argmax(PT.q_values(sd, te, s))  # stays on the device
        PT.tsf_update(sd, te, s, a, r, s1, gamma, as_tensors=True)

    out1, out2 = torch.empty(1, net.d, device=dev), torch.empty(2, net.d, device=dev)
    legs = dict(lib_step=(lib_step, args.window), eager_step=(eager_step, args.eager_window),
                phi_forward_one_row=(lambda: eng.phi_features(s, a1, s1, out=out1), args.window),
                phi_forward_b2=(lambda: eng.phi_features(s2, a2, s12, out=out2), args.window))
    res = {}
    for name, (fn, window) in legs.items():
        for _ in range(args.warmup if name != "eager_step" else 5):
            fn()
        torch.cuda.synchronize()
        res[name] = stats(windows_us(fn, args.windows, window))
    # kernel time alone: the dispatch packets' own timestamps, a leg of its own
    kern = {}
    eng.prof_enable(True)
    for name in ("lib_step", "phi_forward_one_row", "phi_forward_b2"):
        fn, n = legs[name][0], 50
        eng.prof_reset()
        for _ in range(n):
            fn()
        col = eng.prof_collect()
        kern[name] = dict(kernel_us=round(sum(v[1] for v in col.values()) / n, 2),
                          launches=round(sum(v[0] for v in col.values()) / n, 2))
    eng.prof_reset()
    eng.prof_enable(False)
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(td.omega_w).all()), losses
    # the two one-row results agree (the same net, the same row)
    eng.phi_features(s2[:1], a2[:1], s12[:1], out=out1)
    eng.phi_features(s2, a2, s12, out=out2)
    agree = float((out1[0] - out2[0]).abs().max())
    assert agree <= 1e-5 * max(1.0, float(out2.abs().max())), agree

    P = net.P_phi
    one, two = res["phi_forward_one_row"]["median"], res["phi_forward_b2"]["median"]
    out = dict(shape=dict(n_s=net.n_s, A=net.A, d=net.d, H=net.H, T=T, hid=net.hid, n_mid=net.n_mid, phi_params=P),
               device=torch.cuda.get_device_name(0),
               arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
               windows=args.windows, window=args.window, eager_window=args.eager_window,
               us_per_call=res, kernel_time_per_call=kern,
               step_speedup_vs_eager=round(res["eager_step"]["median"] / res["lib_step"]["median"], 2),
               phi_bytes=4 * P,
               one_row_effective_TB_per_s=round(4.0 * P / (one * 1e-6) / 1e12, 3),
               b2_effective_TB_per_s=round(4.0 * P / (two * 1e-6) / 1e12, 3),
               one_row_speedup_vs_b2=round(two / one, 2),
               one_row_kernel_TB_per_s=round(4.0 * P / (kern["phi_forward_one_row"]["kernel_us"] * 1e-6) / 1e12, 3),
               b2_kernel_TB_per_s=round(4.0 * P / (kern["phi_forward_b2"]["kernel_us"] * 1e-6) / 1e12, 3),
               one_row_vs_b2_max_abs_diff=agree)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
    assert not math.isnan(out["step_speedup_vs_eager"])


if __name__ == "__main__":
    main()
