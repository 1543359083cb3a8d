#!/usr/bin/env python3
"""Time one TSF-DQN-with-learned-φ update (sfx_tsf_phi_update) at the width of
main_tsfdqn_phi_torch.py: φ net 13 -> 2048 x4 -> 12 (12.6 M fp32 parameters), n_s = 6, A = 9, d = 12,
ψ heads 256 x 2, T = 4, B = 32.  In one process, on one GPU:

  * library:  median µs per update over --reps graph replays after warm-up (the entry point captures
              its launch chain the second time it sees a key; fixed input buffers keep the key fixed);
  * eager:    the same update in torch eager on the same GPU (tests/tsf_phi_ref.py moved to the device:
              autograd, clamp, a freshly built Adam's step; its results stay on the device, so like the
              library call it makes no host read);
  * floor:    4 passes over the φ net's weights (forward, dX, dW read + write) x 4 B x P / 8 TB/s;
              times_floor = library median / floor.

Writes one JSON object (--out, default profiles/tsf_phi_bench.json) and prints it.
Usage:  python tools/tsf_phi_bench.py [--reps 300] [--eager-reps 30]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "deep-successor-features-for-transfer_amd")):
    sys.path.insert(0, os.path.abspath(p))

from tests import tsf_phi_ref as TP  # noqa: E402

HBM_BYTES_PER_S = 8e12


def problem(net, T, seed=0):
    from sfx.init import reference_heads

    online, w = reference_heads(T, net.n_s, net.H, net.A, net.d, net.acts, seed=seed)
    torch.manual_seed(seed + 1)
    phi0 = torch.cat([torch.cat([m.weight.detach().reshape(-1), m.bias.detach()])
                      for m in (torch.nn.Linear(i, o) for o, i in net.phi_dims)])
    g = torch.stack([torch.cat([m.weight.detach().reshape(-1), m.bias.detach()])
                     for m in (torch.nn.Linear(net.n_s, net.d) for _ in range(T))])
    hm = torch.nn.Linear(net.d, net.d)
    h = torch.cat([hm.weight.detach().reshape(-1), hm.bias.detach()])
    return TP.State(net, online.clone(), online.clone(), w.clone(), torch.zeros(T), phi0, g, h, torch.ones(T))


def events_us(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--eager-reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hid", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsf_phi_bench.json"))
    args = ap.parse_args()
    from sfx.engine import SFEngine

    net, T, B = TP.Net(6, 256, 9, 12, ("relu", "relu"), args.hid, 3), 4, 32
    st = problem(net, T)
    dev = torch.device("cuda", 0)
    eng = SFEngine(T, net.n_s, net.H, net.A, net.d, net.acts, max_batch=B, device="cuda:0")
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
    s, s1 = torch.randn(B, net.n_s, generator=gen).to(dev), torch.randn(B, net.n_s, generator=gen).to(dev)
    a = torch.randint(0, net.A, (B,), generator=gen).to(dev)
    r = torch.rand(B, generator=gen).to(dev)
    gamma = torch.full((B,), 0.9).to(dev)
    wb, lam = torch.zeros(T, device=dev), torch.ones(T, device=dev)
    losses = torch.empty(4, device=dev)

    def lib_update():
        eng.tsf_phi_update(0, s, a, r, s1, gamma, wb[0:1], lam[0:1], use_gpi=True, losses=losses)

    for _ in range(args.warmup):
        lib_update()
    torch.cuda.synchronize()
    lib = events_us(lib_update, args.reps)
    assert bool(torch.isfinite(losses).all()), losses

    sd = st.to(device=dev)
    batch = (s, a, r.reshape(B, 1), s1, gamma)

    def eager_update():
        TP.update(sd, batch, 0, use_gpi=True, target_update_ev=10 ** 9, as_tensors=True)  # no host read

    for _ in range(5):
        eager_update()
    torch.cuda.synchronize()
    eager = events_us(eager_update, args.eager_reps)

    P = net.P_phi
    floor = 4 * 4.0 * P / HBM_BYTES_PER_S * 1e6
    med_lib, med_eager = statistics.median(lib), statistics.median(eager)
    out = dict(shape=dict(n_s=net.n_s, A=net.A, d=net.d, H=net.H, T=T, B=B, hid=net.hid, n_mid=net.n_mid, phi_params=P),
               device=torch.cuda.get_device_name(0),
               arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), reps=args.reps, eager_reps=args.eager_reps,
               lib_us_median=round(med_lib, 2), lib_us_min=round(min(lib), 2),
               lib_us_p90=round(sorted(lib)[int(0.9 * len(lib))], 2),
               eager_us_median=round(med_eager, 2), eager_us_min=round(min(eager), 2),
               byte_floor_us=round(floor, 2), times_floor=round(med_lib / floor, 2),
               speedup_vs_eager=round(med_eager / med_lib, 2))
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
