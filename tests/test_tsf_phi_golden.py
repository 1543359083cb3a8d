"""tests/tsf_phi_ref.py (the torch-autograd restatement of agents/tsfdqn_phi.py
TSFDQN_PHI.update_deep_models) against golden vectors from the real reference
(tests/golden/upd_tsf_phi_{gpi,nogpi}.npz, tools/gen_golden_tsf_phi.py).  CPU only.

Losses to 1e-4 relative.  Parameters: every update is a fresh Adam's first step, ±lr for any
gradient well above ε, so an entry whose gradient is at rounding level may go the other way:
params_close with lr_steps = lr·k bounds those by 2·lr per step, at most 2e-3 of a group."""
import pytest
import torch

from tests import tsf_phi_ref as TP
from tests.test_gpu_engine import params_close, rel_close


@pytest.mark.parametrize("case", ["tsf_phi_gpi", "tsf_phi_nogpi"])
def test_restatement_matches_reference(golden, case):
    g = golden("upd_" + case)
    st = TP.problem_of(g)
    assert st.phi.numel() == st.net.P_phi and st.online.shape[1] == st.net.P_psi
    k = int(g["k"])
    for j, b in enumerate(TP.batches_of(g)):
        out = TP.update(st, b, int(g["policies"][j]), use_gpi=bool(g["use_gpi"]),
                        target_update_ev=int(g["target_update_ev"]))
        print(case, j, out[:4], list(g["losses"][j]))
        rel_close(list(out[:4]), g["losses"][j], rtol=1e-4, atol=1e-7)
    ref = TP.final_of(g, st)
    for name in ("online", "target", "w", "wb", "phi", "g", "h"):
        params_close(getattr(st, name), getattr(ref, name), 1e-3 * k, max_bad_frac=2e-3)
    rel_close(st.lam, ref.lam, rtol=1e-6, atol=1e-7)


def test_update_without_transform_is_the_phi_oracle(golden):
    """transform=False restates oracle/ref_cpu.py phi_update (DeepSF_PHI.update_successor) for a free
    hidden width: at hid = 2 (2 n_s + 1) both must agree on the upd_phi_gpi golden run."""
    from oracle import ref_cpu as R
    from tests.test_oracle_golden import phi_batches, phi_problem

    g = golden("upd_phi_gpi")
    so = phi_problem(g)
    net = TP.Net(so.spec.n_s, so.spec.H, so.spec.A, so.spec.d, tuple(so.spec.acts), 2 * (2 * so.spec.n_s + 1), 3)
    T = so.online.shape[0]
    st = TP.State(net, so.online.clone(), so.target.clone(), so.w.clone(), so.wb.clone(), so.phi.clone(),
                  torch.zeros(T, net.d * net.n_s + net.d), torch.zeros(net.d * net.d + net.d), so.lam.clone())
    for j, b in enumerate(phi_batches(g)):
        i = int(g["policies"][j])
        ref = R.phi_update(so, b, i, use_gpi=True, target_update_ev=int(g["target_update_ev"]))
        s, a, r, _, s1, gamma = b
        out = TP.update(st, (s, a, r, s1, gamma), i, use_gpi=True, target_update_ev=int(g["target_update_ev"]),
                        transform=False)
        assert torch.equal(out[4], ref[4])
        rel_close(list(out[:4]), list(ref[:4]), rtol=1e-6, atol=1e-9)
    for name in ("online", "target", "w", "wb", "phi", "lam"):
        rel_close(getattr(st, name), getattr(so, name), rtol=1e-5, atol=1e-7)
