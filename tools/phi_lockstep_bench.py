#!/usr/bin/env python3
"""Time the SF-φ agent's lockstep test step (agents/sfdqn_phi.py test_agent for E test tasks at once) at the shape
of tools/phi_test_phase_bench.py: φ net 13 -> 2048 x4 -> 12 (12.6 M fp32 parameters), n_s = 6, A = 9, d = 12,
ψ heads 256 x 2, T = 4.  In one process, on one GPU, for E in {1, 2, 4, 8}:

  (a) rows:     the E-row φ chain, sfx_phi_features_rows (csrc/sfx_phitest.h k_phiE_fwd, k_phiE_fwd_lds);
  (b) one_row:  E one-row chains, sfx_phi_features at B = 1 called E times (k_phi1_fwd);
  (c) mfma:     sfx_phi_features at B = E, the update's MFMA forward (k_phiw_fwd) -- not bit-equal to (b); null
                at E = 1, where that call is the one-row GEMV of (b);
  (d) step:     one lockstep step, sfx_phi_test_actions + sfx_phi_test_updates, against E sequential steps of
                DeepSF_PHI.GPI_w's arithmetic (sfx_gpi, the bias add and the argmaxes in torch, on the device) +
                sfx_phi_test_update, both as test env-steps/s of the GPU's part (no env, no host read).

(b) and (c) are the library's existing paths, the yardsticks.  Nothing is read back inside a timed window; a
window is --window calls between two device events, the figure the median over --windows windows after warm-up.

Writes one JSON object (--out, default profiles/phi_lockstep.json) and prints it.
Usage:  python tools/phi_lockstep_bench.py [--windows 15] [--window 40]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in (ROOT, os.path.join(ROOT, "deep-successor-features-for-transfer_amd")):
    sys.path.insert(0, os.path.abspath(p))

from tests import tsf_phi_ref as TP  # noqa: E402
from tools.phi_test_phase_bench import problem, stats, windows_us  # noqa: E402

ROWS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hid", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phi_lockstep.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("phi_lockstep_bench needs a GPU")
    from sfx.engine import SFEngine

    net, T = TP.Net(6, 256, 9, 12, ("relu", "relu"), args.hid, 3), 4
    st, _ = problem(net, T)
    dev = torch.device("cuda", 0)
    eng = SFEngine(T, net.n_s, net.H, net.A, net.d, net.acts, max_batch=32, device="cuda:0")
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    for t in range(T):
        eng.load_head(t, st.online[t], 0)
        eng.load_head(t, st.target[t], 1)
        eng.load_w(t, st.w[t])
    eng.phi_setup_dims(net.hid, net.n_mid, 1e-3)
    eng.phi_load(st.phi)
    gen = torch.Generator().manual_seed(3)
    Emax = max(ROWS)
    S, S1 = torch.randn(Emax, net.n_s, generator=gen).to(dev), torch.randn(Emax, net.n_s, generator=gen).to(dev)
    a = torch.randint(0, net.A, (Emax,), generator=gen).to(dev)
    r = torch.rand(Emax, generator=gen).to(dev)
    W0 = torch.empty(Emax, net.d).uniform_(-0.01, 0.01, generator=gen).to(dev)
    Wb0 = torch.empty(Emax).uniform_(-0.3, 0.3, generator=gen).to(dev)
    r_host = r.tolist()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        return stats(windows_us(fn, args.windows, args.window))

    res = {}
    for E in ROWS:
        s, s1, ae = S[:E].contiguous(), S1[:E].contiguous(), a[:E].contiguous()
        out = torch.empty(E, net.d, device=dev)
        out1 = torch.empty(1, net.d, device=dev)
        rows = [(s[e], ae[e:e + 1], s1[e]) for e in range(E)]

        def one_rows():
            for x, y, z in rows:
                eng.phi_features(x, y, z, out=out1)

        # at E = 1 sfx_phi_features is the one-row GEMV itself, leg (b): no MFMA figure there
        leg = dict(rows=timed(lambda: eng.phi_features_rows(s, ae, s1, out=out)), one_row=timed(one_rows),
                   mfma=timed(lambda: eng.phi_features(s, ae, s1, out=out)) if E > 1 else None)
        # the rows are the one-row kernel's, bit for bit
        got = eng.phi_features_rows(s, ae, s1).clone()
        for e, (x, y, z) in enumerate(rows):
            assert torch.equal(got[e], eng.phi_features(x, y, z)[0]), (E, e)
        # (d) the step
        W, Wb, re, L = W0[:E].clone(), Wb0[:E].clone(), r[:E].contiguous(), torch.empty(E, device=dev)

        def lock_step():
            act = eng.phi_test_actions(s, W, Wb)
            eng.phi_test_updates(s, act[:, 1], re, s1, W, Wb, losses=L)

        Ws = [W0[e].clone() for e in range(E)]
        Wbs = [Wb0[e:e + 1].clone() for e in range(E)]
        l1 = torch.empty(1, device=dev)

        def seq_steps():
            for e in range(E):
                _, q, _, _ = eng.gpi(s[e:e + 1], w=Ws[e])
                q = q + Wbs[e].reshape(1, 1, 1)
                c = torch.squeeze(torch.argmax(torch.max(q, dim=2).values, dim=1))
                act = torch.argmax(q[:, c, :])
                eng.phi_test_update(s[e], act, r_host[e], s1[e], Ws[e], Wbs[e], loss=l1)

        lock, seq = timed(lock_step), timed(seq_steps)
        assert bool(torch.isfinite(W).all()) and bool(torch.isfinite(torch.stack(Ws)).all())
        leg.update(lockstep_step=lock, sequential_steps=seq,
                   lockstep_env_steps_per_s=round(E / (lock["median"] * 1e-6)),
                   sequential_env_steps_per_s=round(E / (seq["median"] * 1e-6)),
                   rows_vs_one_row=round(leg["one_row"]["median"] / leg["rows"]["median"], 2),
                   rows_vs_mfma=round(leg["mfma"]["median"] / leg["rows"]["median"], 2) if leg["mfma"] else None,
                   rows_effective_TB_per_s=round(4.0 * net.P_phi / (leg["rows"]["median"] * 1e-6) / 1e12, 3))
        res[f"E{E}"] = leg
    out = dict(shape=dict(n_s=net.n_s, A=net.A, d=net.d, H=net.H, T=T, hid=net.hid, n_mid=net.n_mid,
                          phi_params=net.P_phi),
               device=torch.cuda.get_device_name(0),
               arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
               windows=args.windows, window=args.window, unit="us per call (median / min / max window)",
               phi_bytes=4 * net.P_phi, rows=res)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
