"""CPU: the comparison tests/test_gpu_adam.py makes is met by the float32 oracle and has teeth.

For every case of the GPU test the float32 oracle's gradient stands in for the one recovered from the GPU.  Then
  * oracle.ref_cpu.adam_ in float32 (torch's own lerp / addcmul / addcdiv kernels) stays within the bound of
    tests/adam_ref.py against the float64 recurrence, at every hyper-parameter set and loaded step count;
  * each mutant of the step leaves the bound on at least one element of every group, at every non-default set and
    every loaded step count (printed: by how much).  One exception, printed and not asserted: on the all-task
    paths, which run at lr_psi / 64 (adam_ref.ALL_TASK_LR), a step count that is off by one at step 2000 moves a
    parameter by about 1e-4 of a 1e-5 step, less than half an ulp of the parameter.  No bound on p' can see that;
    the same two mutants are caught there at the loaded step counts 0 and 3, where the neighbouring heads' bias
    corrections differ by tens of percent, and at step 2000 on every single-head path;
  * the all-task cases keep their next actions when the earlier heads take a measured step (the recovery run leaves
    them where they were), which the GPU test asserts again on the heads it reads back.
"""
import functools
import math

import pytest
import torch

from tests import adam_ref as A
from tests import grad_ref as G

SINGLE = ("ragged16", "one_hidden", "two_row_tiles", "split_n_dx", "three_hidden", "wide_fan_in")
ALL_TASK = ("ragged16", "many_heads", "c2")
TSF = [(K, B, gpi) for K in (0, 3) for B in (7, 32) for gpi in (True, False)]
PHI = (G.PhiCase(26, 32, 3, "mul"), G.PhiCase(136, 32, 3, "dims"))


def psi_case(cid):
    return next(c for c in G.PSI_CASES if c.id == cid)


@functools.lru_cache(maxsize=None)
def groups_of(label):
    """{group: (p, g, floor)} of one case, from the float32 oracles of tests/grad_ref.py."""
    kind, *rest = label.split(":")
    if kind == "update":
        c, gpi = psi_case(rest[0]), rest[1] == "gpi"
        st, (b, _) = G.psi_problem(c)
        g, _ = G.sf_grads(st, c.spec, b, c.T - 1, gpi)
        return dict(psi=(st["online"][c.T - 1], g["psi"], None), w=(st["w"][c.T - 1], g["w"], None))
    if kind == "all":
        c, t = psi_case(rest[0]), int(rest[1])
        st, (b, _) = G.psi_problem(c)
        s, a, _, phi, s1, gamma = b
        g, _ = G.sf_grads(st, c.spec, (s, a, None, phi, s1, gamma), t, True)
        return dict(psi=(st["online"][t], g["psi"], None))
    if kind == "tsf":
        K, B, gpi = int(rest[0]), int(rest[1]), rest[2] == "gpi"
        spec, gs, st, batches, _ = G.tsf_problem(K, B, G.TSF_SEEDS.get((K, B), 0))
        g, _ = G.tsf_grads(st, spec, gs, batches[0], 1, gpi, G.TSF_BETA)
        return dict(psi=(st["online"][1], g["psi"], None), w=(st["w"][1], g["w"], None), g=(st["g"][1], g["g"], None),
                    h=(st["h"], g["h"], None))
    if kind == "tsf_test":
        K = int(rest[0])
        spec, gs, st, _, test = G.tsf_problem(K, 7, G.TSF_SEEDS.get((K, 7), 0))
        s, a, r, phi, s1, a1 = test["steps"][0]
        g = G.tsf_test_grads(st, spec, gs, test["w"], test["omega"], s, a, r, phi, s1, a1, **G.TSF_TEST_HYPER)
        return dict(w=(test["w"], g["w"], None), omega=(test["omega"], g["omega"], 1e-7))
    if kind == "phi":
        c = next(x for x in PHI if x.id == rest[0])
        st, b = G.phi_problem(c, G.PHI_SEEDS.get(c.id, 0))
        g, _ = G.phi_grads(st, b, 1, True, rest[1] == "tsf")
        return dict(psi=(st.online[1], g["psi"], None))
    raise KeyError(label)


LABELS = ([f"update:{c}:{m}" for c in SINGLE for m in ("gpi", "own")]
          + [f"all:{c}:{t}" for c in ALL_TASK for t in (0, psi_case(c).T - 1)]
          + [f"tsf:{K}:{B}:{'gpi' if gpi else 'own'}" for K, B, gpi in TSF]
          + [f"tsf_test:{K}" for K in (0, 3)]
          + [f"phi:{c.id}:{m}" for c in PHI for m in ("sf", "tsf")])


@pytest.mark.parametrize("label", LABELS)
def test_oracle_meets_bound_and_mutants_leave_it(label):
    for gi, (group, (p, g, floor)) in enumerate(groups_of(label).items()):
        for hp, k0 in A.RUNS:
            hp = hp.all_task() if label.startswith("all:") else hp
            s = A.step_of(group, p, g, hp, k0, seed=gi)
            e = A.expect_of(s, floor)
            got = s.run()
            if floor is not None:
                got["p"].clamp_(floor)
            A.check(f"{label} {hp.id} k0={k0} (float32 oracle)", group, got, e)
            if hp.id == A.DEFAULTS.id:
                continue
            for name, fn in A.MUTANTS.items():
                mut = s.run(fn)
                if floor is not None:
                    mut["p"].clamp_(floor)
                r = max(x for x, _ in A.worst(mut, e).values())
                print(f"mutant {name}: {label} {group} {hp.id} k0={k0}: {r:.3g} x the bound")
                if label.startswith("all:") and k0 > 3 and name in ("stale_step", "neighbour_step"):
                    continue   # printed only: see the module docstring
                assert r > 1.0, f"mutant {name} passes on {label} {group} at {hp.id}, k0={k0} ({r:.3g} x the bound)"


def test_expectation_is_the_kernels_recurrence():
    """expect() against a literal float64 transcription on a handful of hand-picked elements, and the narrowing:
    the constants are float32 values, the bias corrections come from doubles."""
    c = A.consts(7e-4, 2e-2, (0.8, 0.9985), 1e-3, 4)
    for k, x in c.items():
        assert x == A.f32(x), k
    assert c["omb1"] == A.f32(1 - 0.8) and c["omb1"] != 1 - 0.8
    assert c["nss"] == A.f32(-(7e-4 / (1 - 0.8 ** 4))) and c["bc2s"] == A.f32(math.sqrt(1 - 0.9985 ** 4))
    p, g, m0, v0 = (torch.tensor(x, dtype=torch.float32) for x in ([0.5, -0.25], [1e-3, 0.0], [2e-3, -1e-3], [4e-6, 1e-6]))
    e = A.expect(p, g, m0, v0, c)
    for j in range(2):
        P, Gr, M0, V0 = (float(x[j]) for x in (p, g, m0, v0))
        Gd = Gr + c["wd"] * P
        M = M0 + c["omb1"] * (Gd - M0)
        V = c["b2"] * V0 + c["omb2"] * Gd * Gd
        want = P + c["nss"] * M / (math.sqrt(V) / c["bc2s"] + c["eps"])
        assert float(e.m[j]) == M and float(e.v[j]) == V and abs(float(e.p[j]) - want) <= 1e-16
    # an element with nothing entering it has a zero bound and must be exact
    z = A.expect(torch.ones(1), torch.zeros(1), torch.zeros(1), torch.zeros(1), A.consts(1e-3, 0.0, (0.9, 0.999), 1e-8, 1))
    assert float(z.bm) == 0 and float(z.bv) == 0 and float(z.m) == 0 and float(z.p) == 1
    assert float(A.ratios(torch.tensor([1e-30]), z.m, z.bm)) == math.inf


def test_hyper_parameter_sets_are_distinct():
    for hp in A.NON_DEFAULT:
        vals = [hp.lr_psi, hp.wd_psi, hp.lr_w, hp.wd_w, hp.lr_g, hp.wd_g, hp.lr_h, hp.wd_h, hp.eps, *hp.betas]
        assert len(set(vals)) == len(vals) and min(vals) > 0
        assert hp.betas != A.DEFAULTS.betas


@pytest.mark.parametrize("cid", ALL_TASK)
def test_all_task_next_actions_survive_a_measured_step(cid):
    """The float32 oracle's all-task step with each non-default set from loaded moments: every head's next actions,
    with the earlier heads moved, are those with the heads unmoved, and the top-2 gap holds in both."""
    c = psi_case(cid)
    st, batches = G.psi_problem(c)
    for hp in A.NON_DEFAULT:
        hp = hp.all_task()
        for k0, b in ((0, 0), (3, 0), (1997, 0), (3, 1)):
            s32 = G.cast(st, torch.float32)
            s, a, _, phi, s1, gamma = batches[b]
            g0 = G.sf_grads(st, c.spec, (s, a, None, phi, s1, gamma), 0, True)[0]["psi"]
            mv = [A.loaded_moments(g0, k0, t) for t in range(c.T)]
            mom = dict(m=torch.stack([m for m, _ in mv]), v=torch.stack([v for _, v in mv]),
                       step=[k0 + t for t in range(c.T)])
            G.all_task_step(s32, mom, c.spec, (s, a, phi, s1, gamma), hp.lr_psi, hp.eps, betas=hp.betas, wd=hp.wd_psi)
            A.assert_next_actions_agree(st, s32["online"], c.spec, s1, f"{cid} {hp.id} k0={k0}")
