"""The Adam step of every update path on the GPU, to a few ulp: decay, betas, ε, loaded moments and step counts.

tests/test_gpu_gradients.py ties the gradient that enters an epilogue to float64 autograd; here the optimizer behind
it is separated from that gradient.  Every case has three runs on one engine and the same inputs:

  1. recovery: zero moments at step 0, every lr = 0, every decay = 0, betas = (0, β2).  The epilogue then computes
     m = fmaf(1, g - 0, 0): the first moments read back through the ABI are the kernel's gradients bit for bit, and
     no parameter moves (p + (-0 m) / denom == p).  Both are asserted;
  2. the recovery again: the moments must be bit-identical (no floating-point atomics, every reduction
     has a fixed order).  A path that were not would have its bound widened by the spread of its two gradients
     pushed through the float64 recurrence (adam_ref.spread), computed here, never a constant;
  3. measured: the same parameters with a hyper-parameter set of tests/adam_ref.py, non-zero moments (m0 at the scale
     of the recovered gradient, v0 > 0 at the scale of its square) and a step count k0 in {0, 3, 1997} (zero moments
     at 0).  p', m', v' of every group the path trains are compared element by element with the float64 recurrence
     on (p, g, m0, v0) under the bound derived in tests/adam_ref.py; the step must read k0 + 1; every head and group
     the path does not train must be bit-identical, moments and step counts (all different) included.

tests/test_adam_ref.py shows on the CPU that torch's own float32 step meets that bound on these cases and that each
of nine mutants of the step (decay left out, decoupled, after the moments; betas exchanged; a stale or a neighbour's
step count; ε under the root; v before the decay; another group's lr / decay) leaves it.

The all-task paths load step k0 + t on head t and run at lr_psi / 64 (adam_ref.ALL_TASK_LR): the recovery run leaves
the earlier heads where they were and the measured run moves them, so the float32 oracle's next actions, with the
heads read back from the GPU in place, are asserted equal to those of the unmoved heads, with the gradient test's
top-2 gap.  Hyper-parameters are baked into captured launches: every case changes them on a live engine (set_adam
clears the graphs; tsf_setup may be called again, it rebuilds the TSF state, which is then reloaded), and one case
runs with and without graphs.

Each printed row is (path, group, output, worst error in units of its bound, that element's magnitude):
profiles/adam_error.md.
"""
import dataclasses

import pytest
import torch

from tests import adam_ref as A
from tests import grad_ref as G
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
NEVER = 10 ** 6   # target sync period: never within a test
OFF = 11          # step-count offset between heads that a single-head path must not mix up


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def dev(x, dtype=torch.float32):
    return torch.as_tensor(x).to("cuda", dtype).contiguous()


def set_hp(eng, hp):
    eng.set_adam(hp.lr_psi, hp.wd_psi, hp.lr_w, hp.wd_w, betas=hp.betas, eps=hp.eps)


def set_recovery(eng, hp=A.DEFAULTS):
    eng.set_adam(0.0, 0.0, 0.0, 0.0, betas=(0.0, hp.betas[1]), eps=hp.eps)


def same(a, b):
    return torch.equal(torch.as_tensor(a).cpu().reshape(-1), torch.as_tensor(b).cpu().reshape(-1))


def recover(run, read_m, read_p, params, what):
    """Runs 1 and 2: -> ({group: g}, {group: g of the repeat}); asserts nothing moved and the repeat is identical."""
    out = []
    for rep in range(2):
        run()
        m = {k: v.clone() for k, v in read_m().items()}
        for k, p in read_p().items():
            assert same(p, params[k]), f"{what}: {k} moved in a step with lr = 0"
        out.append(m)
    for k in out[0]:
        assert bool(torch.isfinite(out[0][k]).all()) and bool(out[0][k].any()), f"{what}: {k} gradient"
        assert same(out[0][k], out[1][k]), f"{what}: the {k} gradient is not reproducible from one run to the next"
    return out


def compare(path, group, got, p, g, g2, m0, v0, lr, wd, hp, step, floor=None):
    c = A.consts(lr, wd, hp.betas, hp.eps, step)
    A.check(path, group, got, A.expect(p, g, m0, v0, c, floor), A.spread(p, g, g2, m0, v0, c, floor))


# ---------------------------------------------------------------------------------------------
# sfx_update: ψ and w of one head
# ---------------------------------------------------------------------------------------------
SINGLE = ("ragged16", "one_hidden", "two_row_tiles", "split_n_dx", "three_hidden", "wide_fan_in")
ALL_TASK = ("ragged16", "many_heads", "c2")


def psi_case(cid):
    return next(c for c in G.PSI_CASES if c.id == cid)


def psi_engine(c):
    from sfx.engine import SFEngine

    spec = c.spec
    eng = SFEngine(c.T, spec.n_s, spec.H, spec.A, spec.d, spec.acts, max_batch=c.max_batch)
    eng.set_target_update_ev(NEVER)
    return eng


def psi_load(eng, st, online, mom, wmom, steps):
    """Heads (online: [T, P]), targets, w, and per head (m, v), (wm, wv), step."""
    for t in range(eng.T):
        eng.load_head(t, online[t], 0)
        eng.load_head(t, st["target"][t], 1)
        eng.load_w_state(t, st["w"][t], *wmom[t])
        eng.load_adam(t, *mom[t], steps[t])


def psi_untouched(eng, st, online, mom, wmom, steps, skip=(), what=""):
    for t in range(eng.T):
        assert same(eng.get_head(t, 1), st["target"][t]), f"{what}: target head {t} moved"
        if t in skip:
            continue
        m, v, k = eng.get_adam(t)
        w, wm, wv = eng.get_w(t)
        assert k == steps[t] and same(m, mom[t][0]) and same(v, mom[t][1]), f"{what}: head {t}'s Adam state changed"
        assert same(eng.get_head(t, 0), online[t]), f"{what}: head {t} moved"
        assert same(w, st["w"][t]) and same(wm, wmom[t][0]) and same(wv, wmom[t][1]), f"{what}: w_{t} changed"


def run_single(eng, c, st, batch, gpi, runs, graphs=None, tag=""):
    """The three runs of sfx_update on head T - 1 -> the measured runs' outputs, for the callers that compare them."""
    i, T = c.T - 1, c.T
    s, a, r, phi, s1, gamma = batch
    zp, zd = torch.zeros(eng.P), torch.zeros(eng.d)
    tag = f"update {c.id}{tag} {'gpi' if gpi else 'own'}"
    if graphs is not None:
        eng.set_graphs(graphs)
        tag += f" graphs={int(graphs)}"

    def rec_run():
        psi_load(eng, st, st["online"], [(zp, zp)] * T, [(zd, zd)] * T, [0] * T)
        eng.update(i, s, a, r, phi, s1, gamma, use_gpi=gpi)
        assert eng.get_adam(i)[2] == 1

    set_recovery(eng)
    g, g2 = recover(rec_run, lambda: dict(psi=eng.get_adam(i)[0], w=eng.get_w(i)[1]),
                    lambda: dict(psi=eng.get_head(i), w=eng.get_w(i)[0]), dict(psi=st["online"][i], w=st["w"][i]), tag)
    outs = []
    for hp, k0 in runs:
        set_hp(eng, hp)
        mom = [A.loaded_moments(g["psi"], k0, 0)] * T
        wmom = [A.loaded_moments(g["w"], k0, 1)] * T
        steps = [k0 + OFF * (i - t) for t in range(T)]
        psi_load(eng, st, st["online"], mom, wmom, steps)
        eng.update(i, s, a, r, phi, s1, gamma, use_gpi=gpi)
        m, v, k = eng.get_adam(i)
        w, wm, wv = eng.get_w(i)
        path = f"{tag} {hp.id} k0={k0}"
        assert k == k0 + 1, f"{path}: step {k}"
        got = dict(psi=dict(p=eng.get_head(i), m=m, v=v), w=dict(p=w, m=wm, v=wv))
        compare(path, "psi", got["psi"], st["online"][i], g["psi"], g2["psi"], *mom[i], hp.lr_psi, hp.wd_psi, hp, k0 + 1)
        compare(path, "w", got["w"], st["w"][i], g["w"], g2["w"], *wmom[i], hp.lr_w, hp.wd_w, hp, k0 + 1)
        psi_untouched(eng, st, st["online"], mom, wmom, steps, skip=(i,), what=path)
        outs.append(got)
    return outs


@pytest.mark.parametrize("gpi", [True, False], ids=["gpi", "own"])
@pytest.mark.parametrize("cid", SINGLE)
def test_update(cid, gpi):
    c = psi_case(cid)
    st, batches = G.psi_problem(c)
    eng = psi_engine(c)
    run_single(eng, c, st, batches[0], gpi, A.RUNS)
    eng.close()


def test_update_graphs_on_and_off():
    """Captured launches carry the hyper-parameters: after set_adam on a live engine the same state gives the new
    set's step (every run_single does that), and the outputs with and without graphs are bit-identical."""
    c = psi_case("ragged16")
    st, batches = G.psi_problem(c)
    eng = psi_engine(c)
    runs = [(A.HP_SETS[1], 3), (A.HP_SETS[2], 3), (A.HP_SETS[1], 3)]
    off = run_single(eng, c, st, batches[0], True, runs, graphs=False)
    on = run_single(eng, c, st, batches[0], True, runs, graphs=True)
    for x, y in zip(off, on):
        for grp in x:
            for k in x[grp]:
                assert same(x[grp][k], y[grp][k]), f"{grp} {k}' differs with graphs"
    for grp in on[0]:   # the first set again after the second: its own result, not the second's
        for k in on[0][grp]:
            assert same(on[0][grp][k], on[2][grp][k]) and not same(on[0][grp][k], on[1][grp][k])
    eng.close()


# ---------------------------------------------------------------------------------------------
# sfx_update_all / sfx_step_all: every head's ψ, head t at step k0 + t
# ---------------------------------------------------------------------------------------------
def heads_of(eng):
    return torch.stack([eng.get_head(t) for t in range(eng.T)])


def all_task_case(c, bf16=False):
    st, batches = G.psi_problem(c)
    spec, T = c.spec, c.T
    eng = psi_engine(c)
    if bf16:
        eng.set_precision("bf16")
    zp, zd = torch.zeros(eng.P), torch.zeros(eng.d)
    wz = [(zd, zd)] * T
    tag = f"update_all {c.id}" + (" bf16" if bf16 else "")
    # bf16: the next actions come from bf16 copies of the heads, which the float32 oracle cannot follow, and an
    # earlier head's move flips some of them (measured: the recovered gradient of a later head then is not the
    # measured run's).  Head 0 sees every head unmoved in both runs, so it alone is compared there; every head's
    # step count still is.
    heads = [0] if bf16 else list(range(T))

    def recovery(online, batch, what):
        s, a, _, phi, s1, gamma = batch

        def rec_run():
            psi_load(eng, st, online, [(zp, zp)] * T, wz, [0] * T)
            eng.update_all(s, a, phi, s1, gamma)
            assert [eng.get_adam(t)[2] for t in range(T)] == [1] * T

        set_recovery(eng)
        g, g2 = recover(rec_run, lambda: {t: eng.get_adam(t)[0] for t in range(T)},
                        lambda: {t: eng.get_head(t) for t in range(T)}, {t: online[t] for t in range(T)}, what)
        return g, g2

    def measured(path, hp, online, mom, steps, g, g2, batch, launch):
        """One measured step from (online, mom, steps) -> (heads, moments) read back."""
        launch(batch)
        got_p = heads_of(eng)
        rd = [eng.get_adam(t) for t in range(T)]
        assert [k for _, _, k in rd] == [k + 1 for k in steps], f"{path}: steps {[k for _, _, k in rd]}"
        if not bf16:
            A.assert_next_actions_agree(dict(online=online, w=st["w"]), got_p, spec, batch[4], path)
        es, ws = [], []
        for t in heads:
            cst = A.consts(hp.lr_psi, hp.wd_psi, hp.betas, hp.eps, steps[t] + 1)
            es.append(A.expect(online[t], g[t], *mom[t], cst))
            ws.append(A.spread(online[t], g[t], g2[t], *mom[t], cst))
        widen = None if all(w is None for w in ws) else A.Expect.cat(
            [w if w is not None else A.Expect(*(torch.zeros_like(e.p),) * 6) for w, e in zip(ws, es)])
        A.check(path, f"psi x{len(heads)}", dict(p=got_p[heads], m=torch.stack([rd[t][0] for t in heads]),
                                                   v=torch.stack([rd[t][1] for t in heads])), A.Expect.cat(es), widen)
        for t in range(T):   # the all-task step trains no w and syncs no target here
            w, wm, wv = eng.get_w(t)
            assert same(w, st["w"][t]) and not wm.any() and not wv.any(), f"{path}: w_{t} changed"
            assert same(eng.get_head(t, 1), st["target"][t]), f"{path}: target head {t} moved"
        return got_p, [(m, v) for m, v, _ in rd]

    def by_update_all(batch):
        s, a, _, phi, s1, gamma = batch
        eng.update_all(s, a, phi, s1, gamma)

    g, g2 = recovery(st["online"], batches[0], tag)
    second = []
    for hp, k0 in A.RUNS:
        hp = hp.all_task()
        set_hp(eng, hp)
        mom = [A.loaded_moments(g[t], k0, t) for t in range(T)]
        steps = [k0 + t for t in range(T)]
        psi_load(eng, st, st["online"], mom, wz, steps)
        p1, mom1 = measured(f"{tag} {hp.id} k0={k0}", hp, st["online"], mom, steps, g, g2, batches[0], by_update_all)
        if k0 == 3 and hp.id != A.DEFAULTS.id and not bf16:
            second.append((hp, p1, mom1, [k + 1 for k in steps]))
    # a second consecutive step on another minibatch, the moments left where the first step put them
    for hp, p1, mom1, steps1 in second:
        ga, gb = recovery(p1, batches[1], f"{tag} {hp.id} second step")
        set_hp(eng, hp)
        psi_load(eng, st, p1, mom1, wz, steps1)
        measured(f"{tag} {hp.id} k0=3 second step", hp, p1, mom1, steps1, ga, gb, batches[1], by_update_all)
    if c.extras and not bf16:
        # sfx_step_all under forced re-runs: speculation, skipped rounds and host rounds leave exactly one step
        gen = torch.Generator().manual_seed(3)
        s_next, lms_phi, lms_r = torch.randn(1, spec.n_s, generator=gen), torch.rand(spec.d, generator=gen), \
            torch.rand(1, generator=gen)

        def by_step_all(batch):
            s, a, _, phi, s1, gamma = batch
            eng.debug_force_rerun(1)
            eng.step_all(dev(s), dev(a, torch.long), dev(phi), dev(s1), dev(gamma), use_gpi=True, lms_task=0,
                         lms_phi=dev(lms_phi), lms_r=dev(lms_r), lms_alpha=0.0, s_next=dev(s_next), task_index=0)
            eng.step_finish()

        for rounds, (hp, k0) in zip((1, 2, 3), ((A.HP_SETS[1], 3), (A.HP_SETS[2], 1997), (A.HP_SETS[1], 0))):
            hp = hp.all_task()
            set_hp(eng, hp)
            eng.set_spec_rounds(rounds)
            mom = [A.loaded_moments(g[t], k0, t) for t in range(T)]
            steps = [k0 + t for t in range(T)]
            psi_load(eng, st, st["online"], mom, wz, steps)
            measured(f"step_all {c.id} rounds={rounds} {hp.id} k0={k0}", hp, st["online"], mom, steps, g, g2, batches[0],
                     by_step_all)
        assert eng.step_stats()["host_round_steps"] >= 3
    eng.close()


@pytest.mark.parametrize("cid", ALL_TASK)
def test_all_task(cid):
    all_task_case(psi_case(cid))


def test_all_task_bf16():
    """bf16 operands change the gradient, not the optimizer: the reference is the GPU's own gradient, so the fp32
    master parameters and moments meet the same bound (head 0 of the all-task step: see all_task_case)."""
    all_task_case(psi_case("c2"), bf16=True)


@pytest.mark.parametrize("gpi", [True, False], ids=["gpi", "own"])
def test_update_bf16(gpi):
    """sfx_update at the flagship shape with bf16 operands: one head trains, so no other head's move enters."""
    c = psi_case("c2")
    st, batches = G.psi_problem(c)
    eng = psi_engine(c)
    eng.set_precision("bf16")
    run_single(eng, c, st, batches[0], gpi, A.RUNS, tag=" bf16")
    eng.close()


# ---------------------------------------------------------------------------------------------
# sfx_tsf_update: ψ_i, w_i, g_i (planar flows + Linear), h with the policy's own moments
# ---------------------------------------------------------------------------------------------
TSF = [(K, B, gpi) for K in (0, 3) for B in (7, 32) for gpi in (True, False)]
TSF_KEYS = dict(psi="online", w="w", g="g", h="h")


def tsf_engine(spec, T):
    from sfx.engine import SFEngine

    eng = SFEngine(T, spec.n_s, spec.H, spec.A, spec.d, spec.acts, max_batch=32)
    eng.set_target_update_ev(NEVER)
    return eng


def tsf_configure(eng, gs, hp, recovery=False):
    """set_adam first (tsf_setup copies betas and ε), then tsf_setup, which rebuilds the TSF state."""
    if recovery:
        set_recovery(eng, hp)
        eng.tsf_setup(gs.G, gs.K, G.TSF_BETA, 0.0, 0.0, 0.0, 0.0)
    else:
        set_hp(eng, hp)
        eng.tsf_setup(gs.G, gs.K, G.TSF_BETA, hp.lr_g, hp.wd_g, hp.lr_h, hp.wd_h)


def tsf_load(eng, st, mom, steps):
    """mom[t] = {group: (m, v)}; h's moments are per policy."""
    for t in range(eng.T):
        eng.load_head(t, st["online"][t], 0)
        eng.load_head(t, st["target"][t], 1)
        eng.load_w_state(t, st["w"][t], *mom[t]["w"])
        eng.load_adam(t, *mom[t]["psi"], steps[t])
        eng.tsf_load_g_state(t, st["g"][t], *mom[t]["g"])
        eng.tsf_load_h_state(t, *mom[t]["h"])
    eng.tsf_load_h(st["h"])


def tsf_read(eng, t):
    m, v, k = eng.get_adam(t)
    w, wm, wv = eng.get_w(t)
    g, gm, gv = eng.tsf_get_g(t)
    hm, hv = eng.tsf_get_h_state(t)
    return dict(psi=dict(p=eng.get_head(t), m=m, v=v), w=dict(p=w, m=wm, v=wv), g=dict(p=g, m=gm, v=gv),
                h=dict(p=eng.tsf_get_h(), m=hm, v=hv)), k


@pytest.mark.parametrize("K,B,gpi", TSF)
def test_tsf_update(K, B, gpi):
    spec, gs, st, batches, _ = G.tsf_problem(K, B, G.TSF_SEEDS.get((K, B), 0))
    T, i = G.TSF_T, 1
    s, a, r, phi, s1, gamma = batches[0]
    eng = tsf_engine(spec, T)
    tag = f"tsf_update K{K} B{B} {'gpi' if gpi else 'own'}"
    params = {k: (st["h"] if k == "h" else st[TSF_KEYS[k]][i]) for k in G.TSF_GROUPS}
    zero = {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in params.items()}

    def rec_run():
        tsf_configure(eng, gs, A.DEFAULTS, recovery=True)
        tsf_load(eng, st, [zero] * T, [0] * T)
        eng.tsf_update(i, s, a, r, phi, s1, gamma, use_gpi=gpi)
        assert eng.get_adam(i)[2] == 1

    g, g2 = recover(rec_run, lambda: {k: x["m"] for k, x in tsf_read(eng, i)[0].items()},
                    lambda: {k: x["p"] for k, x in tsf_read(eng, i)[0].items()}, params, tag)
    nfl = K * (2 * spec.n_s + 1)
    runs = [(hp, k0, False) for hp, k0 in A.RUNS] + ([(A.HP_SETS[1], 3, True)] if K else [])
    for hp, k0, freeze in runs:
        tsf_configure(eng, gs, hp)
        if freeze:
            eng.tsf_freeze_flows(True)
        # every policy its own moments of everything, h included; the steps all differ
        mom = [{k: A.loaded_moments(g[k], k0, 10 * t + j) for j, k in enumerate(G.TSF_GROUPS)} for t in range(T)]
        steps = [k0 + OFF * abs(i - t) for t in range(T)]
        tsf_load(eng, st, mom, steps)
        eng.tsf_update(i, s, a, r, phi, s1, gamma, use_gpi=gpi)
        path = f"{tag} {hp.id} k0={k0}" + (" frozen flows" if freeze else "")
        got, k = tsf_read(eng, i)
        assert k == k0 + 1, f"{path}: step {k}"
        for grp in G.TSF_GROUPS:
            lr, wd = hp.of(grp)
            cst = A.consts(lr, wd, hp.betas, hp.eps, k0 + 1)
            e = A.expect(params[grp], g[grp], *mom[i][grp], cst)
            w = A.spread(params[grp], g[grp], g2[grp], *mom[i][grp], cst)
            if grp == "g" and freeze:   # the flows hold still, decay or not; the Linear of g_i takes its step
                assert same(got["g"]["p"][:nfl], st["g"][i][:nfl]), f"{path}: a frozen flow moved"
                A.check(path, "g Linear", {x: y[nfl:] for x, y in got["g"].items()}, e.sl(nfl, None),
                        None if w is None else w.sl(nfl, None))
            else:
                A.check(path, grp, got[grp], e, w)
        for t in range(T):
            assert same(eng.get_head(t, 1), st["target"][t])
            if t == i:
                continue
            other, k = tsf_read(eng, t)
            assert k == steps[t], f"{path}: policy {t}'s step {k}"
            for grp in ("psi", "w", "g"):
                assert same(other[grp]["p"], st[TSF_KEYS[grp]][t]), f"{path}: policy {t}'s {grp} moved"
            for grp in G.TSF_GROUPS:   # h's moments too: policy i's update leaves another policy's alone
                assert same(other[grp]["m"], mom[t][grp][0]) and same(other[grp]["v"], mom[t][grp][1]), \
                    f"{path}: policy {t}'s {grp} moments changed"
    eng.close()


@pytest.mark.parametrize("K", [0, 3])
def test_tsf_test_update(K):
    """sfx_tsf_test_update: w and ω (clamped at 1e-7) from the caller's state tensor at step k0 + 1."""
    spec, gs, st, _, test = G.tsf_problem(K, 7, G.TSF_SEEDS.get((K, 7), 0))
    d, T = spec.d, G.TSF_T
    eng = tsf_engine(spec, T)
    s, a, r, phi, s1, a1 = test["steps"][0]
    hy = G.TSF_TEST_HYPER
    zero = {k: (torch.zeros(eng.P if k == "psi" else n), ) * 2 for k, n in
            (("psi", 0), ("w", d), ("g", gs.P), ("h", d * gs.G + d))}
    tag = f"tsf_test_update K{K}"

    def call(w, om, state, step, lr_w, wd_w, lr_o, wd_o):
        eng.tsf_test_update(dev(s), dev(s1), dev(a, torch.long), dev(a1, torch.long), r, dev(phi), w, om, state, step,
                            hy["gamma"], hy["beta"], hy["lasso"], lr_w, wd_w, lr_o, wd_o)

    box = {}

    def rec_run():
        tsf_configure(eng, gs, A.DEFAULTS, recovery=True)
        tsf_load(eng, st, [zero] * T, [0] * T)
        box["w"], box["om"], box["state"] = dev(test["w"]), dev(test["omega"]), torch.zeros(2 * (d + T), device="cuda")
        call(box["w"], box["om"], box["state"], 1, 0.0, 0.0, 0.0, 0.0)

    g, g2 = recover(rec_run, lambda: dict(w=box["state"].cpu()[:d], omega=box["state"].cpu()[2 * d:2 * d + T]),
                    lambda: dict(w=box["w"].cpu(), omega=box["om"].cpu()), dict(w=test["w"], omega=test["omega"]), tag)
    before = tsf_read(eng, 1)[0]
    for hp, k0 in A.RUNS:
        tsf_configure(eng, gs, hp)
        tsf_load(eng, st, [zero] * T, [0] * T)
        mw, vw = A.loaded_moments(g["w"], k0, 0)
        mo, vo = A.loaded_moments(g["omega"], k0, 1)
        w, om, state = dev(test["w"]), dev(test["omega"]), dev(torch.cat([mw, vw, mo, vo]))
        (lr_w, wd_w), (lr_o, wd_o) = hp.of("w"), hp.of("omega")
        call(w, om, state, k0 + 1, lr_w, wd_w, lr_o, wd_o)
        now = state.cpu()
        path = f"{tag} {hp.id} k0={k0}"
        compare(path, "w", dict(p=w.cpu(), m=now[:d], v=now[d:2 * d]), test["w"], g["w"], g2["w"], mw, vw, lr_w, wd_w, hp,
                k0 + 1)
        compare(path, "omega", dict(p=om.cpu(), m=now[2 * d:2 * d + T], v=now[2 * d + T:]), test["omega"], g["omega"],
                g2["omega"], mo, vo, lr_o, wd_o, hp, k0 + 1, floor=1e-7)
        after = tsf_read(eng, 1)[0]   # the test phase trains nothing of the source tasks
        for grp in after:
            for k in after[grp]:
                assert same(after[grp][k], before[grp][k]), f"{path}: the source tasks' {grp} {k} changed"
    eng.close()


# ---------------------------------------------------------------------------------------------
# learned φ: the persistent Adam of the ψ head, and the fresh-Adam groups' betas
# ---------------------------------------------------------------------------------------------
PHI = (G.PhiCase(26, 32, 3, "mul"), G.PhiCase(136, 32, 3, "dims"))
PHI_LR = 1e-3
FRESH_ROUNDINGS = 12   # see test_phi_psi_head's docstring


def phi_load(eng, st, tsf, mom, steps):
    T = st.online.shape[0]
    for t in range(T):
        eng.load_head(t, st.online[t], 0)
        eng.load_head(t, st.target[t], 1)
        eng.load_w(t, st.w[t])
        eng.load_adam(t, *mom[t], steps[t])
    eng.phi_load(st.phi)
    if tsf:
        for t in range(T):
            eng.tsf_load_g(t, st.g[t])
        eng.tsf_load_h(st.h)


@pytest.mark.parametrize("transform", [False, True], ids=["phi", "tsf_phi"])
@pytest.mark.parametrize("case", PHI, ids=lambda c: c.id)
def test_phi_psi_head(case, transform):
    """sfx_phi_update / sfx_tsf_phi_update build every optimizer afresh per update, as the reference does
    (features/deep_phi.py, agents/tsfdqn_phi.py): the ψ head's step runs from zero moments at step 1 whatever was
    loaded (k_phi_fresh resets them; the loaded moments and step k0 here must leave no trace), on (lr_psi, wd_psi);
    the other groups (φ net, w, its bias, λ, g_i, h) take the φ setup's lr, no decay, and betas and ε from set_adam.

    At step 1 from zero moments the betas cancel in exact arithmetic (Δ = -lr g / (|g| + ε)), but not bit for bit:
    omb1, omb2, bc2s and nss are narrowed (4 roundings), m = fl(omb1 g), fl(omb2 g), fl(. g), the root, its division
    by bc2s, the sum with ε, fl(nss m) and the quotient round once each (8 more).  Two runs that differ only in the
    betas therefore agree on p' within 2 (u |p'| + 12 u |p' - p|); bit-identity is reported, not required."""
    from sfx.engine import SFEngine

    st, (s, a, r, s1, gamma) = G.phi_problem(case, G.PHI_SEEDS.get(case.id, 0))
    net, T, i = st.net, st.online.shape[0], 1
    eng = SFEngine(T, net.n_s, net.H, net.A, net.d, net.acts, max_batch=case.max_batch)
    eng.set_target_update_ev(NEVER)
    set_recovery(eng)
    if case.setup == "dims":
        eng.phi_setup_dims(net.hid, net.n_mid, PHI_LR)
    else:
        eng.phi_setup(net.hid // (2 * net.n_s + 1), net.n_mid, PHI_LR)
    if transform:
        eng.tsf_setup(net.d, 0)
    fn = eng.tsf_phi_update if transform else eng.phi_update
    zp = torch.zeros(eng.P)
    tag = f"{'tsf_phi' if transform else 'phi'}_update {case.id}"
    box = {}

    def update():
        box["wb"], box["lam"] = dev(st.wb), dev(st.lam)
        fn(i, s, a, r, s1, gamma, box["wb"][i:i + 1], box["lam"][i:i + 1], use_gpi=True)

    def fresh():
        out = dict(phi=eng.phi_get(), w=eng.get_w(i)[0], wb=box["wb"].cpu(), lam=box["lam"].cpu())
        if transform:
            out.update(g=eng.tsf_get_g(i)[0], h=eng.tsf_get_h())
        return out

    def rec_run():
        phi_load(eng, st, transform, [(zp, zp)] * T, [0] * T)
        update()
        assert eng.get_adam(i)[2] == 1

    g, g2 = recover(rec_run, lambda: dict(psi=eng.get_adam(i)[0]), lambda: dict(psi=eng.get_head(i)),
                    dict(psi=st.online[i]), tag)
    before = dict(phi=st.phi, w=st.w[i], wb=st.wb, lam=st.lam, g=st.g[i], h=st.h)
    by_betas = {}
    betas_runs = [(dataclasses.replace(A.DEFAULTS, id="defaults, betas of a", betas=A.HP_SETS[1].betas), 3)]
    for hp, k0 in A.RUNS + betas_runs:
        set_hp(eng, hp)
        mom = [A.loaded_moments(g["psi"], k0, 0)] * T
        steps = [k0 + OFF * abs(i - t) for t in range(T)]
        phi_load(eng, st, transform, mom, steps)
        update()
        m, v, k = eng.get_adam(i)
        path = f"{tag} {hp.id} k0={k0}"
        assert k == 1, f"{path}: step {k}"
        compare(path, "psi", dict(p=eng.get_head(i), m=m, v=v), st.online[i], g["psi"], g2["psi"], zp, zp, hp.lr_psi,
                hp.wd_psi, hp, 1)
        for t in range(T):
            if t != i:
                mt, vt, kt = eng.get_adam(t)
                assert kt == steps[t] and same(mt, mom[t][0]) and same(vt, mom[t][1]) and same(eng.get_head(t), st.online[t])
        if hp.eps == A.DEFAULTS.eps and k0 == 3:
            by_betas[hp.betas] = fresh()
    x, y = by_betas[A.DEFAULTS.betas], by_betas[A.HP_SETS[1].betas]
    for k in x:
        p0, xa, ya = (torch.as_tensor(t).double().reshape(-1) for t in (before[k], x[k], y[k]))
        assert bool((xa != p0).any()), f"{tag}: {k} did not train"
        bound = 2 * A.GUARD * A.U * (xa.abs() + FRESH_ROUNDINGS * (xa - p0).abs())
        r_ = A.ratios(ya, xa, bound)
        j = int(r_.argmax())
        print(f"| {tag} betas a vs defaults | {k} (fresh Adam) | p' | {float(r_[j]):.3f} | {float(xa[j].abs()):.2e} |"
              f" {'bit-identical' if same(x[k], y[k]) else 'to rounding'}")
        assert float(r_[j]) <= 1.0, f"{tag}: {k} depends on the betas ({float(r_[j]):.3g} bounds)"
    eng.close()
