#!/usr/bin/env python3
"""Golden vectors of TSF-DQN with a learned φ, from the REAL reference: agents/tsfdqn_phi.py
TSFDQN_PHI.update_deep_models (:180-288) over features/deep_tsf_phi.py DeepSF_TSF_PHI, on the CPU.

Like tools/gen_golden.py (whose reference import, ψ factory and batch stream it reuses) this runs
only where the reference is present and never on the GPU box; the fixtures are data only:

  tests/golden/upd_tsf_phi_gpi.npz    8 updates, GPI next actions, target sync every 3
  tests/golden/upd_tsf_phi_nogpi.npz  6 updates, own-ψ next actions

Shape: SHAPES["tanh_odd"], T = 3, B = 32, φ net hid = 136 (no multiple of 2 n_s + 1 = 13), n_mid = 3,
policies rotating (3 j) % T.  Recorded: inputs, initial ψ / w / bias / φ / g / h, per-update
(loss, psi_loss, phi_loss, λ), final ψ online and target, w, bias, φ, g, h, λ.

Usage:  python tools/gen_golden_tsf_phi.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG  # noqa: E402  (installs the reference on sys.path)
from agents import tsfdqn_phi as ref_agent  # noqa: E402
from features import deep_tsf_phi as ref_deep  # noqa: E402

HID, N_MID = 136, 3


class Task(GG.SynthTask):
    def action_dim(self):
        return 1


class _NoBuffer:
    def reset(self):
        pass


def phi_lambda(s_enc_dim, action_dim, n_features):
    """main_tsfdqn_phi_torch.py's phi_model_lambda at hidden width HID (the script's is 2048)."""
    n_in = 2 * s_enc_dim + action_dim
    layers = [torch.nn.Linear(n_in, HID), torch.nn.ReLU()]
    for _ in range(N_MID):
        layers += [torch.nn.Linear(HID, HID), torch.nn.ReLU()]
    return torch.nn.Sequential(*layers, torch.nn.Linear(HID, n_features)), torch.nn.MSELoss(), None


def gen(name, shape, T, k, use_gpi, target_update_ev):
    torch.manual_seed(950 + int(use_gpi))
    n_s, H, A, d, acts = shape
    sf = ref_deep.DeepSF_TSF_PHI(pytorch_model_handle=GG.psi_lambda(H, acts), use_true_reward=False,
                                 target_update_ev=target_update_ev)
    agent = ref_agent.TSFDQN_PHI(sf, phi_lambda, _NoBuffer, 0.9, 10, "none", use_gpi=use_gpi)
    agent.reset()
    for t in range(T):
        agent.add_training_task(Task(n_s, A, d, t))
    pm = agent.phi[0][0]
    flat, np_ = GG.flat, GG.np_
    stack = lambda mods: torch.stack([flat(m) for m in mods])
    rec = dict(n_s=n_s, H=H, A=A, d=d, T=T, acts=np.array(acts), k=k, use_gpi=int(use_gpi), hid=HID, n_mid=N_MID,
               target_update_ev=target_update_ev,
               online0=np_(stack([sf.psi[t][0][0] for t in range(T)])),
               w0=np_(torch.stack([sf.fit_w[t].weight.detach().reshape(-1).clone() for t in range(T)])),
               wb0=np_(torch.stack([sf.fit_w[t].bias.detach().reshape(-1).clone() for t in range(T)]).reshape(-1)),
               phi0=np_(flat(pm)), g0=np_(stack(agent.g_functions)), h0=np_(flat(agent.h_function)))
    batches = GG.batch_stream(n_s, A, d, 32, k, torch.Generator().manual_seed(23))
    sb = GG.stack_batches(batches)
    del sb["b_phi"]  # φ is learned: update_deep_models ignores the buffer's features
    rec.update(sb)
    out, policies = [], []
    for j, b in enumerate(batches):
        i = (3 * j) % T
        policies.append(i)
        agent.set_active_training_task(i)
        loss, psi_loss, phi_loss, lam = agent.update_deep_models(b, agent.phi, i, agent.loss_coefficient, use_gpi)
        out.append([float(loss), float(psi_loss), float(phi_loss), float(lam)])
    rec.update(policies=np.array(policies), losses=np.array(out),
               online=np_(stack([sf.psi[t][0][0] for t in range(T)])),
               target=np_(stack([sf.psi[t][1][0] for t in range(T)])),
               w=np_(torch.stack([sf.fit_w[t].weight.detach().reshape(-1).clone() for t in range(T)])),
               wb=np_(torch.stack([sf.fit_w[t].bias.detach().reshape(-1).clone() for t in range(T)]).reshape(-1)),
               phi=np_(flat(pm)), g=np_(stack(agent.g_functions)), h=np_(flat(agent.h_function)),
               lam=np.array([float(x) for x in agent.loss_coefficients]))
    path = os.path.join(GG.OUT, f"upd_{name}.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes")


def main():
    torch.set_num_threads(4)
    gen("tsf_phi_gpi", GG.SHAPES["tanh_odd"], 3, 8, True, 3)
    gen("tsf_phi_nogpi", GG.SHAPES["tanh_odd"], 3, 6, False, 1000)


if __name__ == "__main__":
    main()
