"""The gradient oracles of tests/grad_ref.py on the CPU, at every shape tests/test_gpu_gradients.py runs:

  (a) the float32 oracle pushed through each recovery recipe stays inside grad_close's floor (so the reference
      alone meets the bound the GPU is held to), and the inputs keep away from the kinks -- this fixes the seeds;
  (b) the manual backward of oracle/ref_cpu.py (backward, g_backward, td_grad; float32) agrees with the float64
      autograd oracles under the same bound;
  (c) teeth: a gradient with one batch row dropped from its sums, or scaled by 1.01, fails grad_close while the
      sign comparison that a parameter check after a fresh-Adam step amounts to still passes -- the gap the
      gradient tests close.
"""
import pytest
import torch

from oracle import ref_cpu as R
from tests import grad_ref as G


def _inside_floor(records):
    for label, g64, r32, info in records:
        if info is not None:
            info.check(label)
        for k, ref in g64.items():
            for name in [k] + (["psi_m"] if k == "psi" and "psi_m" in r32 else []):
                _, e32, scale = G.grad_bound(ref, r32[name])
                print(f"| {label} {name} | - | {e32:.2e} | {scale:.2e} |")
                assert scale > 0 and e32 <= G.FLOOR * scale, (label, name, e32, scale)
                assert r32[name].numel() == ref.numel()


# ---- (a) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.PSI_CASES, ids=lambda c: c.id)
def test_psi_reference_inside_floor(case):
    records = G.psi_records(case)
    _inside_floor(records)
    n = (4 if case.single else 0) if case.huber else (2 if case.single else 0)
    assert len(records) == n + case.T * (3 if case.huber else 2)


@pytest.mark.parametrize("K,B,gpi", G.TSF_CASES)
def test_tsf_reference_inside_floor(K, B, gpi):
    records = G.tsf_records(K, B, gpi)
    _inside_floor(records)
    assert [set(g64) for _, g64, _, _ in records] == [set(G.TSF_GROUPS)] * 2
    if B == 7 and gpi:
        _inside_floor(G.tsf_test_records(K))


@pytest.mark.parametrize("transform", [True, False])
@pytest.mark.parametrize("gpi", [True, False])
@pytest.mark.parametrize("case", G.PHI_CASES, ids=lambda c: c.id)
def test_phi_reference_inside_floor(case, gpi, transform):
    records = G.phi_records(case, gpi, transform)
    _inside_floor(records)
    (_, g64, _, info), = records
    assert set(g64) == set(G.TSF_PHI_GROUPS if transform else G.PHI_GROUPS)
    # the ψ epilogue leaves the clamp out: the large-ε recipe must not reach it there (nor anywhere, here)
    assert info.psi_max < 1 and not any(info.clamped.values())


def test_clamp_case_reaches_the_clamp():
    records = G.phi_records(G.CLAMP_CASE, True, True)
    _inside_floor(records)
    (_, g64, _, info), = records
    G.check_clamp_case(info)
    for k in ("phi", "w", "wb", "g", "h"):
        assert float(g64[k].abs().max()) == 1.0


@pytest.mark.parametrize("hid,d", G.PHI_TEST_CASES)
def test_phi_test_phase_reference_inside_floor(hid, d):
    records = G.phi_test_records(hid, d)
    _inside_floor(records)
    assert set(records[0][1]) == {"omega_w", "omega_b", "w", "wb", "lam"} and set(records[1][1]) == {"w", "wb"}


def test_recovery_recipes_invert_adam():
    gen = torch.Generator().manual_seed(0)
    g = torch.randn(1000, generator=gen, dtype=torch.float64) * torch.logspace(-6, 1, 1000, dtype=torch.float64)
    p = torch.randn(1000, generator=gen, dtype=torch.float64)
    for ascent in (False, True):
        assert torch.allclose(G.grad_from_step(p, G.fresh_step(p, g, ascent), ascent), g, rtol=1e-9, atol=1e-14)
    m1, v1 = torch.zeros_like(g), torch.zeros_like(g)
    R.adam_(p.clone(), g, m1, v1, 1, 1e-3)
    assert torch.allclose(G.grad_from_moments(m1), g, rtol=1e-12, atol=0)
    assert torch.allclose(G.second_moment_of(g), v1, rtol=1e-12, atol=0)
    m2, v2 = m1.clone(), v1.clone()
    R.adam_(p.clone(), 3 * g, m2, v2, 2, 1e-3)
    assert torch.allclose(G.grad_from_moments(m2, m1), 3 * g, rtol=1e-9, atol=0)
    assert torch.allclose(G.second_moment_of(3 * g, v1), v2, rtol=1e-12, atol=0)


# ---- (b) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,huber", [(G.PSI_CASES[0], 0.0), (G.PSI_CASES[0], G.HUBER), (G.PSI_CASES[8], G.HUBER),
                                        (G.PSI_CASES[9], 0.0)], ids=lambda x: getattr(x, "id", str(x)))
def test_manual_backward_vs_float64_autograd(case, huber):
    """oracle/ref_cpu.py backward + td_grad, as sf_update runs them (float32), through recipe 1."""
    spec, i = case.spec, case.T - 1
    st, (b, _) = G.psi_problem(case)
    g64, r32, info = G.psi_single_oracles(case, True, huber)
    ref = R.SFState(spec, st["online"].clone(), st["target"].clone(), st["w"].clone())
    *_, nxt = R.sf_update(ref, b, i, use_gpi=True, huber=huber)
    assert torch.equal(nxt, info.next)
    assert ref.step[i] == 1
    G.grad_close(f"manual {case.id} psi", G.grad_from_moments(ref.m[i]), g64["psi"], r32["psi"])
    G.grad_close(f"manual {case.id} w", G.grad_from_moments(ref.wm[i]), g64["w"], r32["w"])
    for m, v in ((ref.m[i], ref.v[i]), (ref.wm[i], ref.wv[i])):
        assert torch.allclose(v.double(), G.second_moment_of(G.grad_from_moments(m)), rtol=1e-5, atol=1e-30)
    # the all-task loop of the same oracle (deep_update), following given next actions, head by head (one step:
    # its Adam has the default ε, the chain's second step starts from ε = 1 parameters)
    steps, _ = G.psi_all_oracles(case, huber, steps=1)
    ref = R.SFState(spec, st["online"].clone(), st["target"].clone(), st["w"].clone())
    prev = ref.m.clone()
    for j, (step, (s, a, _, phi, s1, gamma)) in enumerate(zip(steps, G.psi_problem(case)[1])):
        out = R.deep_all_task_step(ref, (s, a, phi, s1, gamma), lr=G.LR_PSI, target_update_ev=10 ** 6, huber=huber,
                                   next_actions=[info.next for _, _, info in step])
        for t, ((g64, r32, info), (_, nxt)) in enumerate(zip(step, out)):
            assert torch.equal(nxt, info.next)
            G.grad_close(f"manual {case.id} all-task step {j + 1} head {t}", G.grad_from_moments(ref.m[t], prev[t]), g64, r32)
        prev = ref.m.clone()


@pytest.mark.parametrize("K", [0, 3, 4])
def test_manual_tsf_backward_vs_float64_autograd(K):
    """oracle/ref_cpu.py tsf_update (backward, g_backward with K planar flows, td_grad; float32)."""
    B, i = 32, 1
    spec, gs, st, (b, _), _ = G.tsf_problem(K, B, G.TSF_SEEDS.get((K, B), 0))
    (g64, r32, info), _ = G.tsf_oracles(K, B, True, G.TSF_SEEDS.get((K, B), 0))
    ref = R.TSFState(spec, st["online"].clone(), st["target"].clone(), st["w"].clone(), gspec=gs, g=st["g"].clone(),
                     h=st["h"].clone())
    *_, nxt = R.tsf_update(ref, b, i, use_gpi=True, beta=G.TSF_BETA)
    assert torch.equal(nxt, info.next)
    for name, m in (("psi", ref.m[i]), ("w", ref.wm[i]), ("g", ref.gm[i]), ("h", ref.hm[i])):
        G.grad_close(f"manual tsf K{K} {name}", G.grad_from_moments(m), g64[name], r32[name])
    assert not ref.hm[0].any() and not ref.hm[2].any()


# ---- (c) ------------------------------------------------------------------------------------
TEETH = G.PhiCase(136, 32, 3, "dims")


def _teeth_problem():
    st, b = G.phi_problem(TEETH, 0)
    g32, info = G.phi_grads(st, b, 1, True, True)
    st64, b64 = st.to(dtype=G.F64), G.cast(b, G.F64)
    g64, _ = G.phi_grads(st64, b64, 1, True, True, next_actions=info.next)
    r32 = {k: G.through_step(G.phi_params(st, 1)[k], v, ascent=k == "lam") for k, v in g32.items()}
    return st64, b64, info, g64, r32


SMALL = ("w", "wb", "g", "h", "lam")


def test_teeth_one_batch_row_dropped():
    """Every batch sum without one row (the 1/B in front kept): percents off in the small groups with no sign
    changed, so the parameter check passes and grad_close does not."""
    st64, b64, info, g64, r32 = _teeth_problem()
    B, p = TEETH.B, G.phi_params(st64, 1)
    keep = torch.ones(B, dtype=torch.bool)
    found = 0
    for row in range(B):
        keep[:] = True
        keep[row] = False
        mut, _ = G.phi_grads(st64, tuple(x[keep] for x in b64), 1, True, True, next_actions=info.next[keep])
        mut = {k: v * (B - 1) / B for k, v in mut.items()}
        if not all(G.params_check(p[k], mut[k], g64[k]) for k in SMALL):
            continue
        found += 1
        for k in G.TSF_PHI_GROUPS:
            rel = float((mut[k] - g64[k]).abs().max() / g64[k].abs().max())
            print(f"row {row} dropped, {k}: the gradient changes by {rel:.2e} of its max")
            with pytest.raises(AssertionError, match="max .got - ref64."):
                G.grad_close(f"teeth row {k}", mut[k], g64[k], r32[k])
    print(f"{found} of {B} rows can be dropped without the parameter check noticing in w, its bias, g_i, h or λ")
    assert found > 0


def test_teeth_one_group_scaled():
    st64, _, _, g64, r32 = _teeth_problem()
    p = G.phi_params(st64, 1)
    for k in G.TSF_PHI_GROUPS:
        assert G.params_check(p[k], 1.01 * g64[k], g64[k]), k
        with pytest.raises(AssertionError, match="max .got - ref64."):
            G.grad_close(f"teeth scale {k}", 1.01 * g64[k], g64[k], r32[k])
        G.grad_close(f"teeth none {k}", g64[k], g64[k], r32[k])
    assert not G.params_check(p["h"], -g64["h"], g64["h"])   # the parameter check does see a sign


def test_grad_close_compares_every_element():
    ref = torch.ones(1000, dtype=torch.float64)
    got = ref.clone()
    got[617] += 2e-5
    with pytest.raises(AssertionError):
        G.grad_close("one element", got, ref)
    with pytest.raises(AssertionError, match="elements"):
        G.grad_close("short", ref[:999], ref)
    with pytest.raises(AssertionError):
        G.grad_close("floor", ref, ref, floor=2e-4)
