"""tests/phi_test_ref.py (the torch-autograd restatement of the learned-φ agents' test phase: agents/tsfdqn_phi.py
get_test_action / update_target_models, agents/sfdqn_phi.py update_test_reward_mapper) against golden vectors
from the real reference (tests/golden/test_{tsf_phi,phi}.npz, tools/gen_golden_phi_test.py).  CPU only.

Actions exact -- the fixtures record every step's top-2 gap of q, at least 2e-5 at |q| <= 0.25, some hundred fp32
ulps -- losses to 1e-5 relative, the final Ω / w / b_w / λ by params_close with lr_steps = lr·k and no entry
allowed out (a fresh Adam's step is ±lr: an entry may differ by 2·lr per step, never more)."""
import numpy as np
import pytest
import torch

from tests import phi_test_ref as PT
from tests.test_gpu_engine import params_close, rel_close

GAP = 2e-5


def test_tsf_phi_restatement_matches_reference(golden):
    g = golden("test_tsf_phi")
    assert float(np.min(g["gap"])) >= GAP and int(g["k"]) >= 8
    st, tt = PT.problem_of(g)
    assert st.phi.numel() == st.net.P_phi and tt.omega_w.shape == (st.net.d, int(g["T"]) * st.net.d)
    k, gamma = int(g["k"]), float(g["gamma"])
    for j, (s, a, r, s1) in enumerate(PT.steps_of(g)):
        got, gap, qmax, losses = PT.tsf_step(st, tt, s, r, s1, gamma)
        print(j, got, a, gap, float(g["gap"][j]), losses, list(g["losses"][j]))
        assert got == a, (j, got, a, gap)
        assert abs(gap - float(g["gap"][j])) <= 1e-6 and abs(qmax - float(g["qmax"][j])) <= 1e-6
        rel_close(list(losses), g["losses"][j], rtol=1e-5, atol=1e-9)
    ref = PT.final_of(g, tt)
    for name, x in tt.groups().items():
        params_close(x, getattr(ref, name), 1e-3 * k)
    assert not torch.equal(tt.omega_w, torch.from_numpy(g["omega_w0"]))


def test_phi_restatement_matches_reference(golden):
    g = golden("test_phi")
    assert float(np.min(g["gap"])) >= GAP and int(g["k"]) >= 8
    st, tt = PT.problem_of(g)
    k = int(g["k"])
    for j, (s, a, r, s1) in enumerate(PT.steps_of(g)):
        got, gap, qmax = PT.sf_greedy(st, tt, s)
        assert got == a, (j, got, a, gap)
        assert abs(gap - float(g["gap"][j])) <= 1e-6 and abs(qmax - float(g["qmax"][j])) <= 1e-6
        loss = PT.sf_update(st, tt, s, a, r, s1)
        rel_close([loss], g["losses"][j], rtol=1e-5, atol=1e-9)
    ref = PT.final_of(g, tt)
    params_close(tt.w, ref.w, 1e-3 * k)
    params_close(tt.wb, ref.wb, 1e-3 * k)


def _cases():
    from tests.test_gpu_phi_test import CASES

    return CASES


@pytest.mark.parametrize("hid,T,A,d,seed", _cases())
def test_small_case_seeds_fp32_vs_float64(hid, T, A, d, seed):
    """The seeds of tests/test_gpu_phi_test.py's small cases: the fp32 restatement against its own float64 run
    (following the fp32 actions) keeps every step's top-2 gap above 1e-4 max |q| and its parameters within the
    cap the GPU test grants (2e-3 of a group, at most one entry of these groups)."""
    from tests.test_gpu_phi_test import GAMMA, K_SMALL, chain, small_problem

    st, tt = small_problem(hid, T, A, d, seed)
    sf_t = tt.to()
    st64, tt64, sf64 = st.to(dtype=torch.float64), tt.to(dtype=torch.float64), tt.to(dtype=torch.float64)
    for j, (s, r, s1, a_sf) in enumerate(chain(st.net, K_SMALL, seed)):
        a, gap, qmax, lo = PT.tsf_step(st, tt, s, r, s1, GAMMA)
        assert gap >= 1e-4 * qmax, (j, gap, qmax)
        a64, gap64, _, lo64 = PT.tsf_step(st64, tt64, s.double(), r, s1.double(), GAMMA, action=a)
        assert a64 == a
        rel_close(list(lo), list(lo64), rtol=1e-5, atol=1e-9)
        rel_close([PT.sf_update(st, sf_t, s, a_sf, r, s1)], [PT.sf_update(st64, sf64, s.double(), a_sf, r, s1.double())],
                  rtol=1e-5, atol=1e-9)
    for name, x in tt.groups().items():
        params_close(x, getattr(tt64, name), 1e-3 * K_SMALL, max_bad_frac=2e-3)
    params_close(sf_t.w, sf64.w, 1e-3 * K_SMALL, max_bad_frac=2e-3)
    params_close(sf_t.wb, sf64.wb, 1e-3 * K_SMALL, max_bad_frac=2e-3)
