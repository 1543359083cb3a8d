"""The single-file learned-φ agents' main phase on sfx's bound classes: replay of the reference's call logs.

tools/gen_phi_singlefile_golden.py ran sfdqn_phi.py's SFDQN and tsfdqn_phi.py's TSFDQN -- the reference's own code,
on the CPU, with the recipe of tests/golden/recipe_phi.py -- through a short pre_train and a short main phase, and
logged every call across the SF boundary, every `self.phi(s, a, s1)` call included
(tests/golden/calls_*_phi_singlefile.npz).  Here the same calls go to what sfx.dropin.bind puts in the user's modules
-- SingleFileDeepSFPhi / SingleFileDeepTSFPhi, whose tasks' get_w raises, and an sfx.pretrain.LearntPhi loaded with
the logged net -- as tests/test_gpu_dropin.py::test_dropin_replays_reference_call_log does for the other stacks, at
that file's tolerances: GPI tasks exact, q / ψ / losses rel_close(rtol=1e-4), final parameters
params_close(1e-3 * steps), counters exact.  Each φ is held to the bound tests/test_gpu_pretrain.py puts on
sfx_pre_features (tests/grad_ref.py grad_close: against float64, the logged float32 φ as the reference's own error).
"""
import numpy as np
import pytest
import torch

from tests import grad_ref as GR
from tests import pretrain_ref as PR
from tests.conftest import gpu_available
from tests.golden import recipe_phi as RP
from tests.golden.recipe import agent_psi_lambda
from tests.test_gpu_dropin import DEV, _load, _w
from tests.test_gpu_engine import params_close, rel_close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def build(stack, g):
    """The bound library class of `stack` with the recipe's hyper-parameters and the logged initial state."""
    from sfx.dropin import bind

    tsf = stack == "tsfdqn_phi"
    c = RP.AGENT_RUN_TSF_PHI if tsf else RP.AGENT_RUN_SEQ_PHI
    handle = agent_psi_lambda(c["H"], c["acts"], c["lr"], DEV)
    if tsf:
        sf = bind.SingleFileDeepTSFPhi(handle, False, target_update_ev=c["target_update_ev"], hyperparameters=c["hp"])
    else:
        sf = bind.SingleFileDeepSFPhi(pytorch_model_handle=handle, target_update_ev=c["target_update_ev"],
                                      hyperparameters=c["hp"])
    sf.reset()
    T, n_s, d = c["T_tasks"], c["n_s"], c["d"]
    gfun, h = [], None
    if tsf:
        G = c["hp"]["g_h_function_dims"]
        h = torch.nn.Linear(G, d).to(DEV)
        _load(h, g["init.h"])
    for t in range(T):
        task = RP.PhiAgentTask(n_s, c["A"], d, t, t, DEV)     # get_w raises
        if tsf:
            gt = torch.nn.Linear(n_s, G).to(DEV)
            _load(gt, g["init.g"][t])
            gfun.append(gt)
            sf.add_training_task(task, None, gt, h)
        else:
            sf.add_training_task(task)
    for t in range(T):
        (m, _, _), (tm, _, _) = sf.psi[t]
        _load(m, g["init.online"][t])
        _load(tm, g["init.target"][t])
        with torch.no_grad():
            list.__getitem__(sf.fit_w, t).weight.copy_(torch.from_numpy(g["init.w"][t]).view(1, -1))
    return sf, c, gfun, h


def learnt_phi(g, c):
    from sfx.pretrain import LearntPhi, PreEngine

    hidden = tuple(int(x) for x in g["final.phi_hidden"])
    eng = PreEngine(c["n_s"], c["d"], c["T_tasks"], hidden, max_batch=32, device=DEV)
    eng.load(torch.from_numpy(g["final.phi_net"]))
    e64 = PR.RefEngine(c["n_s"], c["d"], c["T_tasks"], hidden, torch.float64)
    e64.load(torch.from_numpy(g["final.phi_net"]))
    return LearntPhi(eng), e64


@pytest.mark.parametrize("stack", ["sfdqn_phi", "tsfdqn_phi"])
def test_dropin_replays_reference_call_log(golden, stack):
    g = golden(f"calls_{stack}_singlefile")
    sf, c, gfun, h = build(stack, g)
    assert not hasattr(sf, "true_w")
    phi, e64 = learnt_phi(g, c)
    names = [str(n) for n in g["names"]]
    counts, got_phi, want64, logged = {}, [], [], []

    def arr(k, key):
        return torch.from_numpy(np.asarray(g[f"c{k}.{key}"])).to(DEV)

    for k, name in enumerate(names):
        counts[name] = counts.get(name, 0) + 1
        if name == "GPI":
            q, task = sf.GPI(arr(k, "state"), int(g[f"c{k}.task_index"]), bool(g[f"c{k}.update_counters"]))
            assert int(task) == int(g[f"c{k}.task"]), f"call {k} (GPI): task {int(task)} vs {int(g[f'c{k}.task'])}"
            rel_close(q, g[f"c{k}.q"], rtol=1e-4, atol=1e-6)
        elif name in ("get_successors", "get_next_successors"):
            rel_close(getattr(sf, name)(arr(k, "state")), g[f"c{k}.psi"], rtol=1e-4, atol=1e-6)
        elif name == "phi":
            s, a, s1 = arr(k, "state"), arr(k, "action"), arr(k, "next_state")
            out = phi(s, a, s1)     # the call form of sfdqn_phi.py:503: 2-d states, a 0-d int64 action
            assert out.device == DEV and tuple(out.shape) == (1, c["d"])
            got_phi.append(out.cpu())
            want64.append(e64.features(s.cpu(), a.cpu().reshape(1), s1.cpu()))
            logged.append(torch.from_numpy(g[f"c{k}.phi"]))
        elif name in ("update_successor", "tsf_update"):
            pi, use_gpi = int(g[f"c{k}.policy_index"]), bool(g[f"c{k}.use_gpi"])
            tr = tuple(arr(k, f"t{i}") for i in range(6)) if bool(g[f"c{k}.has_batch"]) else None
            if name == "tsf_update":
                out = None if tr is None else sf.tsf_update(tr, pi, use_gpi, beta=c["hp"]["beta_loss_coefficient"])
            else:
                out = sf.update_successor(tr, pi, use_gpi)
            if f"c{k}.losses" in g:
                rel_close(torch.stack([torch.as_tensor(x).float().cpu() for x in out]), g[f"c{k}.losses"], rtol=1e-4,
                          atol=1e-7)
            else:
                assert out is None
        else:
            raise AssertionError(f"unknown call {name}")
    steps = counts.get("update_successor", 0) + counts.get("tsf_update", 0)
    assert counts.get("GPI", 0) > 0 and steps > 0 and counts["phi"] >= steps
    GR.grad_close(f"{stack} learnt_phi, {len(got_phi)} calls", torch.cat(got_phi), torch.cat(want64), torch.cat(logged))
    T = sf.n_tasks
    online = torch.stack([torch.cat([p.detach().reshape(-1).cpu() for p in sf.psi[t][0][0].parameters()])
                          for t in range(T)])
    target = torch.stack([torch.cat([p.detach().reshape(-1).cpu() for p in sf.psi[t][1][0].parameters()])
                          for t in range(T)])
    params_close(online, g["final.online"], 1e-3 * steps)
    params_close(target, g["final.target"], 1e-3 * steps)
    rel_close(torch.stack([_w(sf.fit_w[t]) for t in range(T)]), g["final.w"], rtol=1e-4, atol=1e-7)
    assert np.array_equal(np.stack([np.asarray(x) for x in sf.gpi_counters]), g["final.gpi_counters"])
    assert list(sf.updates_since_target_updated) == [int(x) for x in g["final.since_target"]]
    if gfun:
        sf.sync_tsf_modules()
        params_close(torch.stack([torch.cat([p.detach().reshape(-1).cpu() for p in m.parameters()]) for m in gfun]),
                     g["final.g"], 1e-3 * steps)
        params_close(torch.cat([p.detach().reshape(-1).cpu() for p in h.parameters()]), g["final.h"], 1e-3 * steps)
    phi.engine.close()
