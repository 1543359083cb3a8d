#!/usr/bin/env python3
"""Golden vectors of the learned-φ agents' test phase, from the REAL reference on the CPU:

  tests/golden/test_tsf_phi.npz  agents/tsfdqn_phi.py TSFDQN_PHI.get_test_action (:381-397) and
                                 update_target_models (:434-505), 10 chained steps
  tests/golden/test_phi.npz      agents/sfdqn_phi.py SFDQN_PHI.get_test_action (:224-232, through GPI_w) and
                                 update_test_reward_mapper (:263-305), 10 chained steps

Like tools/gen_golden_tsf_phi.py (whose reference import, φ net at hid 136 and synthetic tasks it reuses) this
runs only where the reference is present and never on the GPU box; the fixtures are data only.

Shape: SHAPES["tanh_odd"], T = 3, hid 136, n_mid 3.  The target heads are the online heads plus noise (after
training they differ), test_epsilon = 0, the test task's reward model initialised as the agents' train() does
(weight ~ U(-0.01, 0.01), torch's default bias).  A chain: s_0 ~ N(0, 1), per step a = get_test_action(s),
s1 ~ N(0, 1), r ~ U(0, 1), the update, s = s1.  Recorded: the heads, the φ net (once: the test phase does not
change it), g, h, the initial and final Ω / w / b_w / λ, per step s, a, r, s1, the top-2 gap of q and max |q|,
and the losses.  Every recorded step's gap is at least GAP, so that the same action is a fair demand on fp32
arithmetic of another summation order; a seed with a narrower gap is dropped for the next one.

Usage:  python tools/gen_golden_phi_test.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_tsf_phi as GT  # noqa: E402  (installs the reference on sys.path)
from agents import sfdqn_phi as ref_sf_agent  # noqa: E402
from features import deep_phi as ref_deep_phi  # noqa: E402

GG, ref_agent, ref_deep = GT.GG, GT.ref_agent, GT.ref_deep
GAP, K, T, GAMMA = 2e-5, 10, 3, 0.9


def test_model(d, gen):
    """The test task's reward model as the agents' train() builds it."""
    w = torch.nn.Linear(d, 1)
    with torch.no_grad():
        w.weight = torch.nn.Parameter(torch.empty(1, d).uniform_(-0.01, 0.01, generator=gen))
    return w


def noisy_targets(sf, T, gen):
    with torch.no_grad():
        for t in range(T):
            for p in sf.psi[t][1][0].parameters():
                p.add_(torch.empty_like(p).uniform_(-0.05, 0.05, generator=gen))


def top2(q):
    q = q.detach().reshape(-1)
    top = torch.topk(q, 2).values
    return float(top[0] - top[1]), float(q.abs().max())


def common(sf, pm, shape, seed):
    n_s, H, A, d, acts = shape
    flat, np_ = GG.flat, GG.np_
    return dict(n_s=n_s, H=H, A=A, d=d, T=T, acts=np.array(acts), k=K, hid=GT.HID, n_mid=GT.N_MID, gamma=GAMMA,
                seed=seed, online=np_(torch.stack([flat(sf.psi[t][0][0]) for t in range(T)])),
                target=np_(torch.stack([flat(sf.psi[t][1][0]) for t in range(T)])), phi=np_(flat(pm)))


def gen_tsf(shape, seed):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 1)
    n_s, H, A, d, acts = shape
    sf = ref_deep.DeepSF_TSF_PHI(pytorch_model_handle=GG.psi_lambda(H, acts), use_true_reward=False,
                                 target_update_ev=1000)
    agent = ref_agent.TSFDQN_PHI(sf, GT.phi_lambda, GT._NoBuffer, GAMMA, 10, "none", use_gpi=True, test_epsilon=0.0)
    agent.reset()
    for t in range(T):
        agent.add_training_task(GT.Task(n_s, A, d, t))
    noisy_targets(sf, T, gen)
    pm = agent.phi[0][0]
    w, lam = test_model(d, gen), agent.init_loss_coefficients()
    flat, np_ = GG.flat, GG.np_
    rec = common(sf, pm, shape, seed)
    rec.update(g=np_(torch.stack([flat(m) for m in agent.g_functions])), h=np_(flat(agent.h_function)),
               omega_w0=np_(agent.omegas.weight), omega_b0=np_(agent.omegas.bias),
               w0=np_(w.weight.reshape(-1)), wb0=np_(w.bias.reshape(-1)), lam0=np_(lam.reshape(-1)))
    phi0 = flat(pm)
    steps = dict(s=[], a=[], r=[], s1=[], gap=[], qmax=[], losses=[])
    s = torch.randn(1, n_s, generator=gen)
    for _ in range(K):
        with torch.no_grad():
            q = w(agent.omegas(sf.get_successors(s).swapaxes(1, 2).flatten(start_dim=2)))
        gap, qmax = top2(q)
        if gap < GAP:
            return None
        a = agent.get_test_action(s, w)
        s1, r = torch.randn(1, n_s, generator=gen), float(torch.rand(1, generator=gen))
        loss, psi_loss, phi_loss = agent.update_target_models(w, lam, r, s, a, s1)
        for name, v in zip(steps, (np_(s[0]), int(a), r, np_(s1[0]), gap, qmax,
                                   [float(x.detach()) for x in (loss, psi_loss, phi_loss)])):
            steps[name].append(v)
        s = s1
    assert torch.equal(flat(pm), phi0)  # the test phase leaves the φ net alone
    rec.update({k: np.array(v) for k, v in steps.items()})
    rec.update(omega_w=np_(agent.omegas.weight), omega_b=np_(agent.omegas.bias), w=np_(w.weight.reshape(-1)),
               wb=np_(w.bias.reshape(-1)), lam=np_(lam.reshape(-1)))
    return rec


def gen_sf(shape, seed):
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed + 1)
    n_s, H, A, d, acts = shape
    sf = ref_deep_phi.DeepSF_PHI(pytorch_model_handle=GG.psi_lambda(H, acts), use_true_reward=False,
                                 target_update_ev=1000)
    agent = ref_sf_agent.SFDQN_PHI(sf, GT.phi_lambda, GT._NoBuffer, GAMMA, 10, "none", use_gpi=True, test_epsilon=0.0)
    agent.reset()
    for t in range(T):
        agent.add_training_task(GT.Task(n_s, A, d, t))
    pm = agent.phi[0][0]
    w = test_model(d, gen)
    np_ = GG.np_
    rec = common(sf, pm, shape, seed)
    rec.update(w0=np_(w.weight.reshape(-1)), wb0=np_(w.bias.reshape(-1)))
    steps = dict(s=[], a=[], r=[], s1=[], gap=[], qmax=[], losses=[])
    s = torch.randn(1, n_s, generator=gen)
    for _ in range(K):
        with torch.no_grad():
            q, c = sf.GPI_w(s, w)
        # the action is the argmax over (task, action): the gap that matters is the one of the whole table
        gap, qmax = top2(q)
        if gap < GAP:
            return None
        a = agent.get_test_action(s, w)
        s1, r = torch.randn(1, n_s, generator=gen), float(torch.rand(1, generator=gen))
        loss = agent.update_test_reward_mapper(w, r, s, a, s1)
        for name, v in zip(steps, (np_(s[0]), int(a), r, np_(s1[0]), gap, qmax, [float(loss.detach())])):
            steps[name].append(v)
        s = s1
    rec.update({k: np.array(v) for k, v in steps.items()})
    rec.update(w=np_(w.weight.reshape(-1)), wb=np_(w.bias.reshape(-1)))
    return rec


def main():
    torch.set_num_threads(4)
    for name, fn in (("test_tsf_phi", gen_tsf), ("test_phi", gen_sf)):
        for seed in range(970, 1000):
            rec = fn(GG.SHAPES["tanh_odd"], seed)
            if rec is not None:
                break
            print(name, "seed", seed, "dropped: a top-2 gap below", GAP)
        assert rec is not None and float(np.min(rec["gap"])) >= GAP
        path = os.path.join(GG.OUT, name + ".npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes; seed", rec["seed"], "gaps", rec["gap"], "max |q|", rec["qmax"])


if __name__ == "__main__":
    main()
