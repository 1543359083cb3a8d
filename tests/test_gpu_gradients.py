"""Gradient VALUES of every update path on the GPU against float64 autograd (tests/grad_ref.py).

The parameter comparisons of the other GPU tests see a gradient through Adam, which hides its size: a persistent
Adam's step is m̂/√v̂, a freshly built one's ±lr.  Here the gradient itself is read back through the ABI --

  1. from the moments a first step leaves (m = (1-β1) g, v = (1-β2) g², step == 1; a second consecutive step through
     g₂ = (m₂ - β1 m₁)/(1-β1)): sfx_update, sfx_update_all, sfx_step_all, sfx_tsf_update, sfx_tsf_test_update, and
     the ψ head of the learned-φ updates;
  2. from one fresh-Adam step with ε = lr = 1 (Δp = -g/(|g| + 1)): sfx_phi_update, sfx_tsf_phi_update,
     sfx_tsf_phi_test_update, sfx_phi_test_update --

and every element of every group is compared by grad_close: max |got - ref64| <= max(4 x the float32 oracle's own
error through the same recovery, 1e-5 max |ref64|).  tests/test_grad_ref.py shows on the CPU that the float32 oracle
meets that floor at every case here and that the inputs keep clear of the ReLU / Huber / clamp kinks; the next
actions the float64 oracle follows are the float32 oracle's, asserted equal to the GPU's wherever the entry point
returns them (the all-task step does not: there the float32 oracle's top-2 gap is asserted instead).
Each printed row is (group, GPU error, float32-reference error, max |g|, bound): profiles/gradient_error.md.
"""
import functools

import pytest
import torch

from tests import grad_ref as G
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
NEVER = 10 ** 6   # target sync period: never within a test


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def dev(x, dtype=torch.float32):
    return torch.as_tensor(x).to("cuda", dtype).contiguous()


def check_v(name, v, g, v_prev=None):
    """The second moment that goes with the recovered gradient."""
    want = G.second_moment_of(g, v_prev).reshape(-1)
    v = torch.as_tensor(v).detach().cpu().double().reshape(-1)
    atol = float(want.max()) * (1e-10 if v_prev is None else 1e-5)
    assert torch.allclose(v, want, rtol=1e-5, atol=atol), f"{name}: v is not (1-β2) g² (max diff {float((v - want).abs().max()):.3e})"


# ---------------------------------------------------------------------------------------------
# ψ paths
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def psi_records(case_id):
    case = next(c for c in G.PSI_CASES if c.id == case_id)
    return {label: (g64, r32, info) for label, g64, r32, info in G.psi_records(case)}


def psi_engine(c, huber=0.0):
    from sfx.engine import SFEngine

    spec = c.spec
    eng = SFEngine(c.T, spec.n_s, spec.H, spec.A, spec.d, spec.acts, max_batch=c.max_batch)
    eng.set_adam(G.LR_PSI, 0.0, G.LR_PSI, 0.0, eps=G.EPS_PSI)
    eng.set_target_update_ev(NEVER)
    if huber:
        eng.set_huber(huber)
    return eng


def psi_load(eng, st):
    """The problem's heads and w with zero moments and step 0."""
    zp, zd = torch.zeros(eng.P), torch.zeros(eng.d)
    for t in range(eng.T):
        eng.load_head(t, st["online"][t], 0)
        eng.load_head(t, st["target"][t], 1)
        eng.load_w_state(t, st["w"][t], zd, zd)
        eng.load_adam(t, zp, zp, 0)


def check_all_task(eng, recs, label, prev=None, step=1):
    """Every head's moments after an all-task step against the oracle; returns them for the next step."""
    out = []
    for t in range(eng.T):
        m, v, k = eng.get_adam(t)
        assert k == step, f"{label} head {t}: step {k}"
        g64, r32, info = recs[f"{label} head {t}"]
        info.check(f"{label} head {t}")
        got = G.grad_from_moments(m, None if prev is None else prev[t][0])
        G.grad_close(f"{label} head {t} psi", got, g64["psi"], r32["psi"])
        check_v(f"{label} head {t}", v, got, None if prev is None else prev[t][1])
        out.append((m, v))
    return out


@pytest.mark.parametrize("case", G.PSI_CASES, ids=lambda c: c.id)
def test_psi_gradients(case):
    recs = psi_records(case.id)
    st, batches = G.psi_problem(case)
    B, i = case.B, case.T - 1
    for hub in (0.0, G.HUBER) if case.huber else (0.0,):
        tag = "huber " if hub else ""
        eng = psi_engine(case, hub)
        s, a, r, phi, s1, gamma = batches[0]
        if case.single:
            nxt = torch.empty(B, dtype=torch.int64, device="cuda")
            for gpi in (True, False):
                label = f"{case.id} {tag}update {'gpi' if gpi else 'own'}"
                g64, r32, info = recs[label]
                psi_load(eng, st)
                eng.update(i, s, a, r, phi, s1, gamma, use_gpi=gpi, next_actions=nxt)
                m, v, step = eng.get_adam(i)
                assert torch.equal(nxt.cpu(), info.next), f"{label}: next actions"
                assert step == 1
                got = G.grad_from_moments(m)
                G.grad_close(f"{label} psi", got, g64["psi"], r32["psi"])
                check_v(label, v, got)
                _, wm, wv = eng.get_w(i)
                got = G.grad_from_moments(wm)
                G.grad_close(f"{label} w", got, g64["w"], r32["w"])
                check_v(label + " w", wv, got)
                m0, v0, step0 = eng.get_adam(0)   # another head: untouched
                assert step0 == 0 and not m0.any() and not v0.any()
        # the all-task step: one step's moments, then a second step on another minibatch
        psi_load(eng, st)
        eng.update_all(s, a, phi, s1, gamma)
        first = check_all_task(eng, recs, f"{case.id} {tag}all-task step 1")
        if not hub:
            s2, a2, _, phi2, s12, gamma2 = batches[1]
            eng.update_all(s2, a2, phi2, s12, gamma2)
            check_all_task(eng, recs, f"{case.id} all-task step 2", prev=first, step=2)
        if case.extras and not hub:
            # speculation, skipped rounds and host rounds leave exactly one step's moments
            gen = torch.Generator().manual_seed(3)
            s_next, lms_phi, lms_r = torch.randn(1, case.spec.n_s, generator=gen), torch.rand(case.spec.d, generator=gen), \
                torch.rand(1, generator=gen)
            for rounds in (1, 2, 3):
                psi_load(eng, st)
                eng.set_spec_rounds(rounds)
                eng.debug_force_rerun(1)
                eng.step_all(dev(s), dev(a, torch.long), dev(phi), dev(s1), dev(gamma), use_gpi=True, lms_task=0,
                             lms_phi=dev(lms_phi), lms_r=dev(lms_r), lms_alpha=0.0, s_next=dev(s_next), task_index=0)
                eng.step_finish()
                assert torch.equal(eng.get_w(0)[0], st["w"][0])   # an LMS fit at rate 0
                check_all_task(eng, recs, f"{case.id} all-task step 1")
            assert eng.step_stats()["host_round_steps"] >= 3
        eng.close()


# ---------------------------------------------------------------------------------------------
# TSF
# ---------------------------------------------------------------------------------------------
def tsf_engine(spec, gs, st, max_batch=32):
    from sfx.engine import SFEngine

    T = st["online"].shape[0]
    eng = SFEngine(T, spec.n_s, spec.H, spec.A, spec.d, spec.acts, max_batch=max_batch)
    eng.set_adam(G.LR_PSI, 0.0, G.LR_PSI, 0.0, eps=G.EPS_PSI)   # before tsf_setup, which copies ε
    eng.set_target_update_ev(NEVER)
    eng.tsf_setup(gs.G, gs.K, G.TSF_BETA, G.LR_PSI, 0.0, G.LR_PSI, 0.0)
    for t in range(T):
        eng.load_head(t, st["online"][t], 0)
        eng.load_head(t, st["target"][t], 1)
        eng.load_w(t, st["w"][t])
        eng.tsf_load_g(t, st["g"][t])
    eng.tsf_load_h(st["h"])
    return eng


@pytest.mark.parametrize("K,B,gpi", G.TSF_CASES)
def test_tsf_gradients(K, B, gpi):
    """Policy 1 on one minibatch, then policy 2 on another: each policy's first step, so its moments of ψ_i, w_i,
    g_i (K planar flows, not frozen) and its own moments of the shared h are (1-β1) g; the second update leaves
    the first policy's h moments alone."""
    spec, gs, st, batches, _ = G.tsf_problem(K, B, G.TSF_SEEDS.get((K, B), 0))
    recs = G.tsf_records(K, B, gpi)
    eng = tsf_engine(spec, gs, st)
    nxt = torch.empty(B, dtype=torch.int64, device="cuda")
    h_first = None
    for (label, g64, r32, info), i, (s, a, r, phi, s1, gamma) in zip(recs, (1, 2), batches):
        info.check(label)
        eng.tsf_update(i, s, a, r, phi, s1, gamma, use_gpi=gpi, next_actions=nxt)
        m, v, step = eng.get_adam(i)
        assert torch.equal(nxt.cpu(), info.next), f"{label}: next actions"
        assert step == 1
        got = dict(psi=(m, v), w=eng.get_w(i)[1:], g=eng.tsf_get_g(i)[1:], h=eng.tsf_get_h_state(i))
        for k in G.TSF_GROUPS:
            g = G.grad_from_moments(got[k][0])
            G.grad_close(f"{label} {k}", g, g64[k], r32[k])
            check_v(f"{label} {k}", got[k][1], g)
        if h_first is None:
            h_first = got["h"]
        else:
            hm, hv = eng.tsf_get_h_state(1)
            assert torch.equal(hm, h_first[0]) and torch.equal(hv, h_first[1]), "policy 2's update touched policy 1's h moments"
        hm, hv = eng.tsf_get_h_state(0)
        assert not hm.any() and not hv.any()
    eng.close()


@pytest.mark.parametrize("K", [0, 2, 3, 4])
def test_tsf_test_update_gradients(K):
    """sfx_tsf_test_update at step 1 and 2 on the same problem: w and ω from the caller's Adam state."""
    spec, gs, st, _, test = G.tsf_problem(K, 7, G.TSF_SEEDS.get((K, 7), 0))
    recs = G.tsf_test_records(K)
    eng = tsf_engine(spec, gs, st)
    d, T = spec.d, G.TSF_T
    w, om = dev(test["w"]), dev(test["omega"])
    state = torch.zeros(2 * (d + T), device="cuda")
    hy = G.TSF_TEST_HYPER
    for k, ((label, g64, r32, _), (s, a, r, phi, s1, a1)) in enumerate(zip(recs, test["steps"])):
        prev = state.cpu().clone()
        eng.tsf_test_update(dev(s), dev(s1), dev(a, torch.long), dev(a1, torch.long), r, dev(phi), w, om, state, k + 1,
                            hy["gamma"], hy["beta"], hy["lasso"], G.LR_PSI, 0.0, G.LR_PSI, 0.0)
        now = state.cpu()
        for name, lo, n in (("w", 0, d), ("omega", 2 * d, T)):
            g = G.grad_from_moments(now[lo:lo + n], prev[lo:lo + n] if k else None)
            G.grad_close(f"{label} {name}", g, g64[name], r32[name])
            check_v(f"{label} {name}", now[lo + n:lo + 2 * n], g, prev[lo + n:lo + 2 * n] if k else None)
    eng.close()


# ---------------------------------------------------------------------------------------------
# learned φ
# ---------------------------------------------------------------------------------------------
def phi_engine(st, c, tsf):
    """ε = lr = 1 for every group (the ψ heads take lr_psi, everything else the φ setup's lr)."""
    from sfx.engine import SFEngine

    net, T = st.net, st.online.shape[0]
    eng = SFEngine(T, net.n_s, net.H, net.A, net.d, net.acts, max_batch=c.max_batch)
    eng.set_adam(1.0, 0.0, 1.0, 0.0, eps=1.0)   # before tsf_setup, which copies ε
    eng.set_target_update_ev(NEVER)
    for t in range(T):
        eng.load_head(t, st.online[t], 0)
        eng.load_head(t, st.target[t], 1)
        eng.load_w(t, st.w[t])
    if c.setup == "dims":
        eng.phi_setup_dims(net.hid, net.n_mid, 1.0)
    else:
        eng.phi_setup(net.hid // (2 * net.n_s + 1), net.n_mid, 1.0)
    eng.phi_load(st.phi)
    if tsf:
        eng.tsf_setup(net.d, 0)
        for t in range(T):
            eng.tsf_load_g(t, st.g[t])
        eng.tsf_load_h(st.h)
    return eng


def run_phi_case(c, gpi, transform, i=1):
    st, (s, a, r, s1, gamma) = G.phi_problem(c, G.PHI_SEEDS.get(c.id, 0))
    (label, g64, r32, info), = G.phi_records(c, gpi, transform)
    info.check(label)
    assert info.psi_max < 1   # the ψ epilogue leaves the clamp out: the large-ε step must not reach it there
    eng = phi_engine(st, c, transform)
    wb, lam = dev(st.wb), dev(st.lam)
    nxt = torch.empty(c.B, dtype=torch.int64, device="cuda")
    fn = eng.tsf_phi_update if transform else eng.phi_update
    fn(i, s, a, r, s1, gamma, wb[i:i + 1], lam[i:i + 1], use_gpi=gpi, next_actions=nxt)
    m, v, step = eng.get_adam(i)
    assert torch.equal(nxt.cpu(), info.next), f"{label}: next actions"
    assert step == 1
    before = G.phi_params(st, i)
    after = dict(psi=eng.get_head(i, 0), phi=eng.phi_get(), w=eng.get_w(i)[0], wb=wb[i:i + 1].cpu(), lam=lam[i:i + 1].cpu())
    if transform:
        after.update(g=eng.tsf_get_g(i)[0], h=eng.tsf_get_h())
    for k in G.TSF_PHI_GROUPS if transform else G.PHI_GROUPS:
        G.grad_close(f"{label} {k}", G.grad_from_step(before[k], after[k], ascent=k == "lam"), g64[k], r32[k])
    got = G.grad_from_moments(m)   # the ψ head again, from the moments its fresh Adam leaves
    G.grad_close(f"{label} psi (moments)", got, g64["psi"], r32["psi_m"])
    check_v(label, v, got)
    for t in range(st.online.shape[0]):   # nothing else moved
        if t != i:
            assert torch.equal(eng.get_head(t, 0), st.online[t]) and torch.equal(eng.get_w(t)[0], st.w[t])
            assert torch.equal(wb[t].cpu(), st.wb[t]) and torch.equal(lam[t].cpu(), st.lam[t])
            if transform:
                assert torch.equal(eng.tsf_get_g(t)[0], st.g[t])
    eng.close()
    return g64, info


@pytest.mark.parametrize("transform", [True, False], ids=["tsf_phi", "phi"])
@pytest.mark.parametrize("gpi", [True, False], ids=["gpi", "own"])
@pytest.mark.parametrize("case", G.PHI_CASES, ids=lambda c: c.id)
def test_phi_gradients(case, gpi, transform):
    _, info = run_phi_case(case, gpi, transform)
    assert not any(info.clamped.values())


def test_tsf_phi_clamped_gradients():
    """Rewards x40: the [-1, 1] clamp bites in the φ net, w, its bias, g_i and h (max |g| = 1 exactly there) and
    not in ψ; a clamp left out, or put on the wrong tensor, changes these gradients by far more than the bound."""
    g64, info = run_phi_case(G.CLAMP_CASE, True, True)
    G.check_clamp_case(info)
    for k in ("phi", "w", "wb", "g", "h"):
        assert float(g64[k].abs().max()) == 1.0


@pytest.mark.parametrize("hid,d", G.PHI_TEST_CASES)
def test_phi_test_phase_gradients(hid, d):
    """sfx_tsf_phi_test_update (Ω weight and bias, w, its bias, λ) and sfx_phi_test_update (w, its bias)."""
    st, tt, (s, a, r, s1) = G.phi_test_problem(hid, d, G.PHI_TEST_SEEDS.get((hid, d), 0))
    (tl, t64, t32, _), (sl, s64, s32, _) = G.phi_test_records(hid, d)
    eng = phi_engine(st, G.PhiCase(hid, 1, 3, "mul" if hid == 26 else "dims", d=d), True)
    td, sd = tt.to(dtype=torch.float32, device="cuda"), tt.to(dtype=torch.float32, device="cuda")
    eng.tsf_phi_test_update(s, a, r, s1, G.GAMMA, td.omega_w, td.omega_b, td.w, td.wb, td.lam)
    for k, before in tt.groups().items():
        G.grad_close(f"{tl} {k}", G.grad_from_step(before, getattr(td, k), ascent=k == "lam"), t64[k], t32[k])
    eng.phi_test_update(s, a, r, s1, sd.w, sd.wb)
    for k in ("w", "wb"):
        G.grad_close(f"{sl} {k}", G.grad_from_step(getattr(tt, k), getattr(sd, k)), s64[k], s32[k])
    assert torch.equal(eng.phi_get(), st.phi) and torch.equal(eng.tsf_get_h(), st.h)   # the test phase trains neither
    eng.close()
