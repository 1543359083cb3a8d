#!/usr/bin/env python3
"""Call logs of the single-file learned-φ agents, from the REAL reference on the CPU: sfdqn_phi.py's SFDQN over
its DeepSF and tsfdqn_phi.py's TSFDQN over its DeepTSF, each through a short pre_train and a short main phase
(tests/golden/recipe_phi.py).

Like tools/gen_golden.py (whose CallLog and recording classes this uses) it runs only where the reference is present
and never on the GPU box; the fixtures are data only.  tests/golden/calls_sfdqn_phi_singlefile.npz and
calls_tsfdqn_phi_singlefile.npz hold the frozen net's parameters (torch packing, `phi_net`) and widths, the library
state before the first call and after the last, and in order every call across the SF boundary with inputs and
outputs -- GPI, get_successors, get_next_successors, update_successor / the TSF agent's own update_successor
(`tsf_update`), and every `self.phi(s, a, s1)` call (`phi`: state, action, next_state, the φ row it returned).

The modules' missing globals are injected as tools/gen_pretrain_golden.py does: `device` (both read it at module
level only under __main__) and tsfdqn_phi's `print_debug` (False, its __main__'s value).

Usage:  python tools/gen_phi_singlefile_golden.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402  (installs the reference read-only, with the tensorboard stub)
from tests.golden import recipe_phi as RP  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def reference(name):
    module = __import__(name)
    module.device = torch.device("cpu")
    module.print_debug = False
    return module


class LoggedPhi:
    """The frozen PhiFunction, every call logged at the SF boundary."""

    def __init__(self, phi, log, sf):
        self.phi, self.log, self.sf = phi, log, sf

    def __call__(self, state, action, next_state):
        return self.log.call(self.sf, "phi", lambda: self.phi(state, action, next_state),
                             lambda o: dict(state=state, action=action, next_state=next_state, phi=o))

    def __getattr__(self, name):
        return getattr(self.phi, name)


def generate(name, module, tsf):
    log = GG.CallLog()
    net = {}

    def pretrained(agent):
        model = agent.learnt_phi._model
        net["phi_net"] = GG.np_(GG.flat(model))
        net["phi_hidden"] = np.array([m.out_features for m in model if isinstance(m, torch.nn.Linear)][:-1])
        agent.learnt_phi = LoggedPhi(agent.learnt_phi, log, agent.sf)

    lib = GG.recording_sf(module.DeepTSF if tsf else module.DeepSF, log)
    with contextlib.redirect_stdout(io.StringIO()):
        if tsf:
            agent, *_ = RP.agent_run_tsf_phi(lib, GG.recording_tsf_agent(module.TSFDQN, log), module.ReplayBuffer,
                                             torch.device("cpu"), pretrained)
        else:
            agent, *_ = RP.agent_run_sequential_phi(lib, module.SFDQN, module.ReplayBuffer, torch.device("cpu"),
                                                    pretrained)
    final = GG._final(agent, log)
    final.update({k: v for k, v in net.items()})
    path = os.path.join(OUT, name + ".npz")
    log.save(path, final)
    names = [n for n, _ in log.calls]
    counts = {n: names.count(n) for n in sorted(set(names))}
    c = RP.AGENT_RUN_TSF_PHI if tsf else RP.AGENT_RUN_SEQ_PHI
    upd = counts.get("tsf_update", 0) + counts.get("update_successor", 0)
    assert upd == c["T_tasks"] * c["n_samples"] and counts["phi"] >= upd, counts
    gpi = [f for n, f in log.calls if n == "GPI"]
    transfers = sum(int(f["task"]) != int(f["task_index"]) for f in gpi)
    assert transfers > 0, "no GPI call chose another task's policy: lengthen the recipe"
    print(path, os.path.getsize(path), "bytes;", counts, "GPI transfers", transfers, "since_target",
          final["since_target"])
    assert os.path.getsize(path) < 1 << 20


def main():
    torch.set_num_threads(1)
    generate("calls_sfdqn_phi_singlefile", reference("sfdqn_phi"), tsf=False)
    generate("calls_tsfdqn_phi_singlefile", reference("tsfdqn_phi"), tsf=True)


if __name__ == "__main__":
    main()
