"""bf16 operand mode by VALUE (DESIGN.md §3 "bf16 operand mode"): every bf16 product the library computes against
the float64 emulation of the same product, one product at a time, operands known exactly (tests/bf16_ref.py; the
mutants each check rejects are in tests/test_bf16_ref.py).

  * forward: carrier heads isolate one layer; ψ read through sfx_successors (online and target parameters),
    sfx_gpi, sfx_select_action (M = 1, one-hot reward weights) and, after one lr = 0 all-task step, from the slot
    its Adam epilogue wrote the copies of;
  * backward: the layer-1 dX from the GPU's own dZ_1, read bit for bit from the first moments of a recovery step;
  * the copies are q(master) after every writer: updates, all-task steps, a TSF update, precision switches, the
    target sync inside an update and sfx_sync_target;
  * the look-ahead forward is the step-start forward, in bf16 as in fp32.

The same probes run in fp32 mode against the fp32 emulation under the same bound: the read-outs are exact, not
loose.  Every case prints its worst error / bound; the table is profiles/bf16_error.md.
"""
import dataclasses

import pytest
import torch

from oracle import ref_cpu as R
from tests import bf16_ref as B
from tests import grad_ref as G
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu
PRECS = ("bf16", "fp32")
NEVER = 1 << 30
ROWS = []


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def profile_table():
    """The table of profiles/bf16_error.md from this run's rows: one line per case, the entry points listed, the
    worst ratio of each mode."""
    import re

    cases = {}
    for case, prec, reaches, entry, ratio, n in ROWS:
        c = cases.setdefault(case, dict(reaches=reaches, entries=[], bf16=0.0, fp32=0.0, n=n))
        c[prec] = max(c[prec], ratio)
        entry = re.sub(r" head \d+| \(w = e_\d+\)", "", entry)
        if entry not in c["entries"]:
            c["entries"].append(entry)
    out = ["| case | instantiation reached | entry points | bf16: worst error / bound | fp32: worst error / bound "
           "| elements |", "|---|---|---|---|---|---|"]
    out += [f"| {k} | `{c['reaches']}` | {', '.join(c['entries'])} | {c['bf16']:.3g} | {c['fp32']:.3g} | {c['n']} |"
            for k, c in cases.items()]
    return "\n".join(out)


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if ROWS:   # pytest -s: the table as profiles/bf16_error.md holds it
        print("\n" + profile_table())


def row(case, prec, reaches, entry, ratio, n, bad):
    ROWS.append((case, prec, reaches, entry, ratio, n))
    assert bad == 0, f"{case} ({prec}) via {entry}: {bad} of {n} elements outside the check, worst error / bound {ratio:.3g}"


def engine(g, T, online, target, prec, max_batch=32, ev=NEVER):
    from sfx.engine import SFEngine

    eng = SFEngine(T, g.n_s, g.H, g.A, g.d, g.acts, max_batch=max_batch)
    eng.set_target_update_ev(ev)
    for t in range(T):
        eng.load_head(t, online[t], 0)
        eng.load_head(t, target[t], 1)
    eng.set_precision(prec)
    return eng


def recovery(eng, T):
    """tests/test_gpu_adam.py's recovery recipe: the first moments of the next step are its gradients."""
    eng.set_adam(0.0, 0.0, 0.0, 0.0, betas=(0.0, 0.999))
    z = torch.zeros(eng.P)
    for t in range(T):
        eng.load_adam(t, z, z, 0)


def some_batch(g, rows, seed):
    gen = torch.Generator().manual_seed(seed)
    s, s1 = torch.rand(rows, g.n_s, generator=gen) + 0.1, torch.rand(rows, g.n_s, generator=gen) + 0.1
    return (s, torch.randint(0, g.A, (rows,), generator=gen), torch.rand(rows, 1, generator=gen),
            torch.rand(rows, g.d, generator=gen), s1, torch.full((rows,), 0.9))


def device_rows(S, aligned):
    """S on the device; not aligned: a view one float off 16-byte alignment."""
    if aligned:
        return S.cuda()
    buf = torch.empty(S.numel() + 1, device="cuda")
    v = buf[1:].view(S.shape)
    v.copy_(S)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("p", B.FWD_PROBES, ids=lambda p: p.id)
def test_forward_product(p, prec):
    g, bf = p.geo, prec == "bf16"
    online, target = B.carrier_heads(p), B.carrier_heads(dataclasses.replace(p, seed=p.seed + 1))
    S = B.probe_inputs(p)
    refs = [B.run_probe(p, h, S, B.F64, bf16=bf) for h in (online, target)]
    eng = engine(g, p.T, online, target, prec, max_batch=32 * -(-p.M // 32))
    Sd = device_rows(S, p.aligned)
    for which, (h, ref) in enumerate(zip((online, target), refs)):   # load_head(which) wrote both copies
        got = eng.successors(Sd, which).cpu()
        row(p.id, prec, p.reaches, f"successors({which})", *B.check_probe(p, h, got, ref))
    first = eng.successors(Sd, 0).cpu()
    eng.load_w(0, torch.eye(g.d)[0])
    psi = eng.gpi(Sd, w_index=0, want_psi=True)[0].cpu()
    row(p.id, prec, p.reaches, "gpi", *B.check_probe(p, online, psi, refs[0]))
    if p.M == 1:   # q = ψ·e_k is ψ[..., k] exactly (an fmaf chain over zeros)
        for k in (0, g.d - 1):
            eng.load_w(1, torch.eye(g.d)[k])
            qd = torch.empty(p.T, g.A, device="cuda")
            eng.select_action(Sd.view(-1), 1, True, q_out=qd)
            eng.synchronize()
            err = (qd.cpu().double() - refs[0].z.view(p.T, g.A, g.d)[..., k]).abs()
            bound = refs[0].bound.view(p.T, g.A, g.d)[..., k]
            row(p.id, prec, p.reaches, f"select_action (w = e_{k})", float((err / bound).max()), err.numel(),
                int((err > bound).sum()))
    # one all-task step with lr = 0: the parameters stay, the Adam epilogue writes the other slot and its copies
    recovery(eng, p.T)
    rows = min(p.M, 32)
    s, a, _, phi, s1, gamma = some_batch(g, rows, 11)
    eng.update_all(s, a, phi, s1, gamma)
    eng.synchronize()
    got = eng.successors(Sd, 0).cpu()
    row(p.id, prec, p.reaches, "successors(0) after update_all", *B.check_probe(p, online, got, refs[0]))
    assert torch.equal(got, first), "ψ moved in a step with lr = 0"
    eng.close()


# ---------------------------------------------------------------------------------------------
# forward: the three groups of sfx_update's own launches (online at s, target at s1, every online head at s1)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("p", B.UPD_PROBES, ids=lambda p: p.id)
def test_update_forward_groups(p, prec):
    """ψ(s) of the online group and ψ⁻(s1) of the target group (read from the target's bf16 copy) out of the last
    bias' first moments after a recovery step: distinct actions per row make every entry a single term
    (tests/bf16_ref.py, "sfx_update's own forward launches")."""
    g, bf, i = p.geo, prec == "bf16", p.T - 1
    online, target = B.carrier_heads(p), B.carrier_heads(dataclasses.replace(p, seed=p.seed + 1))
    S = B.probe_inputs(p)
    r_on, r_tg = (B.run_probe(p, h, S, B.F64, bf16=bf) for h in (online, target))
    eng = engine(g, p.T, online, target, prec)
    eng.load_w(i, torch.linspace(-0.5, 0.5, g.d))
    zero, rows = torch.zeros(p.M, g.d), torch.arange(p.M)
    r = torch.zeros(p.M, 1)
    worst, bad, n = 0.0, 0, 0
    for rot in range(g.A):   # the online group: φ = 0, γ = 0; every action of every row in turn
        a = (rows + rot) % g.A
        recovery(eng, p.T)
        eng.update(i, S, a, r, zero, S.flip(0), torch.zeros(p.M), use_gpi=rot % 2 == 0)
        ratio, k, b = B.upd_verdict(p, eng.get_adam(i)[0], a, a, r_on.z[:, i], r_on.bound[:, i], 1.0)
        worst, bad, n = max(worst, ratio), bad + b, n + k
    row(p.id, prec, p.reaches, "update: online group at s", worst, n, bad)
    # the target group: ψ(s) = 0 exactly (s = 0, no last bias in the online head), φ = 0, γ = 1
    w1 = g.offsets()[-1][1]
    quiet = online[i].clone()
    quiet[w1:w1 + g.A * g.d] = 0
    eng.load_head(i, quiet, 0)
    for gpi in (True, False):
        a = (rows * 3 + 1) % g.A if g.A % 3 else rows
        nxt = torch.empty(p.M, dtype=torch.int64, device="cuda")
        recovery(eng, p.T)
        eng.update(i, torch.zeros_like(S), a, r, zero, S, torch.ones(p.M), use_gpi=gpi, next_actions=nxt)
        ratio, k, b = B.upd_verdict(p, eng.get_adam(i)[0], a, nxt.cpu(), r_tg.z[:, i], r_tg.bound[:, i], -1.0)
        row(p.id, prec, p.reaches, f"update ({'GPI' if gpi else 'own'}): target group at s1", ratio, k, b)
    eng.close()


# ---------------------------------------------------------------------------------------------
# target parameters: every path that writes them
# ---------------------------------------------------------------------------------------------
SYNC = B.Probe("sync_last_H64", B.G2(17, 64), 3, 17, 3, "target copy")


@pytest.mark.parametrize("prec", PRECS)
def test_sync_target_carries_the_copy(prec):
    """After sfx_sync_target the target forward is the online forward, bit for bit -- in bf16 mode the target's
    bf16 copy has to follow the fp32 parameters."""
    p = SYNC
    online, target = B.carrier_heads(p), B.carrier_heads(dataclasses.replace(p, seed=9))
    S = B.probe_inputs(p)
    ref = B.run_probe(p, online, S, B.F64, bf16=prec == "bf16")
    eng = engine(p.geo, p.T, online, target, prec)
    before = eng.successors(S, 1).cpu()
    for t in (0, 2):
        eng.sync_target(t)
    on, tg = eng.successors(S, 0).cpu(), eng.successors(S, 1).cpu()
    assert torch.equal(tg[:, 0], on[:, 0]) and torch.equal(tg[:, 2], on[:, 2])
    assert torch.equal(tg[:, 1], before[:, 1]) and not torch.equal(tg[:, 1], on[:, 1])   # head 1 was not synced
    for t in (0, 2):
        assert torch.equal(eng.get_head(t, 1), online[t])
    tg[:, 1] = on[:, 1]
    row(p.id, prec, p.reaches, "successors(1) after sync_target", *B.check_probe(p, online, tg, ref))
    eng.close()


@pytest.mark.parametrize("prec", PRECS)
def test_target_sync_inside_update_carries_the_copy(prec):
    """target_update_ev = 1: the update of head 1 ends with its target sync (lr = 0: the parameters stay)."""
    p = SYNC
    online, target = B.carrier_heads(p), B.carrier_heads(dataclasses.replace(p, seed=9))
    S = B.probe_inputs(p)
    ref = B.run_probe(p, online, S, B.F64, bf16=prec == "bf16")
    eng = engine(p.geo, p.T, online, target, prec, ev=1)
    recovery(eng, p.T)
    eng.update(1, *some_batch(p.geo, 17, 12))
    on, tg = eng.successors(S, 0).cpu(), eng.successors(S, 1).cpu()
    assert torch.equal(tg[:, 1], on[:, 1]) and not torch.equal(tg[:, 0], on[:, 0])
    tg[:, 0], tg[:, 2] = on[:, 0], on[:, 2]
    row(p.id, prec, p.reaches, "successors(1) after update's sync", *B.check_probe(p, online, tg, ref))
    eng.close()


# ---------------------------------------------------------------------------------------------
# backward: the layer-1 dX
# ---------------------------------------------------------------------------------------------
TSF_PROBE = B.BwdProbe("tsf_K0_ns32_H64", B.G2(32, 64, 4, 8), 2, 17, "tsf_update", "k_bwd_tsf<NP,true> psi part")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("p", B.BWD_PROBES + [TSF_PROBE], ids=lambda p: p.id)
def test_layer1_dx(p, prec):
    g, bf = p.geo, prec == "bf16"
    heads, target, (s, a, r, phi, s1, gamma), i, j = B.bwd_problem(p)
    eng = engine(g, p.T, heads, target, prec, max_batch=p.max_batch)
    for t in range(p.T):
        eng.load_w(t, torch.linspace(-0.5, 0.5, g.d))
    if p.entry == "tsf_update":
        gs = R.GSpec(g.n_s, 5, 0)
        gen = torch.Generator().manual_seed(3)
        eng.set_adam(0.0, 0.0, 0.0, 0.0, betas=(0.0, 0.999))   # before tsf_setup, which copies ε
        eng.tsf_setup(gs.G, gs.K, 0.5, 0.0, 0.0, 0.0, 0.0)
        for t in range(p.T):
            eng.tsf_load_g(t, torch.empty(gs.P).uniform_(-0.3, 0.3, generator=gen))
        eng.tsf_load_h(torch.empty(g.d * gs.G + g.d).uniform_(-0.4, 0.4, generator=gen))
    recovery(eng, p.T)
    if p.entry == "update_all":
        eng.update_all(s, a, phi, s1, gamma)
        updated = range(p.T)
    else:
        (eng.tsf_update if p.entry == "tsf_update" else eng.update)(p.T - 1, s, a, r, phi, s1, gamma)
        updated = [p.T - 1]
    eng.synchronize()
    (w0, w1) = g.offsets()[1]
    for t in updated:
        m, _, step = eng.get_adam(t)
        assert step == 1 and torch.equal(eng.get_head(t, 0), heads[t]), "a parameter moved in a step with lr = 0"
        dz1, dz0, db1 = B.bwd_readout(p, m, i, j)
        assert bool(dz1.any()) and bool(dz0.any())
        ref, bound = B.dx_reference(p, heads[t, w0:w1].view(g.H, g.H), dz1, bf)
        row(p.id, prec, p.reaches, f"{p.entry} head {t}", *B.dx_verdict(dz0, ref, bound))
        db = B.db_verdict(dz1, db1)
        print(f"{p.id} ({prec}) head {t}: db_1 error / bound {db:.3g}")
        assert db <= 1.0, f"{p.id}: db_1 is not the column sum of the dZ_1 read from dW_1 ({db:.3g} bounds)"
        if bf:   # and the fp32 product of the same bits is outside: the bound tells the two apart
            assert B.dx_verdict(dz0, *B.dx_reference(p, heads[t, w0:w1].view(g.H, g.H), dz1, False))[2] > 0
    eng.close()


# ---------------------------------------------------------------------------------------------
# the copies are q(master) after every writer
# ---------------------------------------------------------------------------------------------
def fresh_equal(eng, g, T, max_batch, S):
    """A fresh bf16 engine loaded with eng's fp32 heads has q(master) copies by construction: bit-equal ψ from both
    parameter sets proves eng's copies are q(master) too."""
    fresh = engine(g, T, [eng.get_head(t, 0) for t in range(T)], [eng.get_head(t, 1) for t in range(T)], "bf16",
                   max_batch=max_batch)
    for which in (0, 1):
        assert torch.equal(fresh.successors(S, which).cpu(), eng.successors(S, which).cpu()), f"which = {which}"
    fresh.close()


def psi_engine(c, ev=NEVER, prec="bf16"):
    st, batches = G.psi_problem(c)
    g = B.Geo(c.spec.n_s, c.spec.H, c.spec.A, c.spec.d, len(c.spec.acts))
    eng = engine(g, c.T, st["online"], st["target"], prec, max_batch=c.max_batch, ev=ev)
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    for t in range(c.T):
        eng.load_w(t, st["w"][t])
    return eng, g, batches


CASES = {c.id: c for c in G.PSI_CASES}


@pytest.mark.parametrize("cid", ["ragged16", "three_hidden"])
def test_copies_after_updates(cid):
    c = CASES[cid]
    eng, g, batches = psi_engine(c, ev=2)   # the second update syncs the target
    for k in range(3):
        eng.update(c.T - 1, *batches[k % 2], use_gpi=k != 1)
    assert not torch.equal(eng.get_head(c.T - 1, 0), eng.get_head(c.T - 1, 1))
    fresh_equal(eng, g, c.T, c.max_batch, batches[0][0])
    eng.close()


@pytest.mark.parametrize("cid", ["ragged16", "one_hidden"])
def test_copies_after_all_task_steps(cid):
    c = CASES[cid]
    eng, g, batches = psi_engine(c, ev=2)
    for k in range(2):
        s, a, _, phi, s1, gamma = batches[k]
        eng.update_all(s, a, phi, s1, gamma)
    eng.synchronize()
    fresh_equal(eng, g, c.T, c.max_batch, batches[0][0])
    eng.close()


def test_copies_after_tsf_update():
    spec, gs, st, batches, _ = G.tsf_problem(0, 7, 0)
    g = B.Geo(spec.n_s, spec.H, spec.A, spec.d, len(spec.acts))
    T = st["online"].shape[0]
    eng = engine(g, T, st["online"], st["target"], "bf16", ev=1)
    eng.set_adam(1e-3, 0.0, 1e-3, 0.0)
    eng.tsf_setup(gs.G, gs.K, G.TSF_BETA, 1e-3, 0.0, 1e-3, 0.0)
    for t in range(T):
        eng.load_w(t, st["w"][t])
        eng.tsf_load_g(t, st["g"][t])
    eng.tsf_load_h(st["h"])
    before = eng.get_head(1, 0)
    eng.tsf_update(1, *batches[0])
    assert not torch.equal(eng.get_head(1, 0), before)
    fresh_equal(eng, g, T, 32, batches[0][0])
    eng.close()


def test_copies_across_precision_switches():
    c = CASES["ragged16"]
    eng, g, batches = psi_engine(c, prec="fp32")
    eng.update(c.T - 1, *batches[0])      # fp32 -> update -> bf16 -> fp32 -> update -> bf16
    eng.set_precision("bf16")
    eng.set_precision("fp32")
    eng.update(c.T - 1, *batches[1])      # the copies of the first switch are stale now
    eng.set_precision("bf16")
    fresh_equal(eng, g, c.T, c.max_batch, batches[0][0])
    eng.close()


def test_copies_after_sync_target():
    c = CASES["ragged16"]
    eng, g, batches = psi_engine(c)
    eng.update(c.T - 1, *batches[0])
    eng.sync_target(c.T - 1)
    S = batches[0][0]
    assert torch.equal(eng.successors(S, 1)[:, c.T - 1].cpu(), eng.successors(S, 0)[:, c.T - 1].cpu())
    fresh_equal(eng, g, c.T, c.max_batch, S)
    eng.close()


# ---------------------------------------------------------------------------------------------
# composition: a whole update against the emulated network
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.COMP_CASES, ids=lambda c: c.id)
def test_whole_update_composes(c):
    """One sfx_update in bf16 mode against tests/grad_ref.py's ψ oracle with the emulated Linear (forward and dX
    maps of tests/bf16_ref.py), by grad_close as it is.  The seeds keep every operand off the bf16 midpoints."""
    (pc, st, b), g64, r32, info, dist = B.comp_oracles(c)
    info.check(c.id)
    assert dist > B.MID
    eng = engine(c.geo, c.T, st["online"], st["target"], "bf16")
    eng.set_adam(G.LR_PSI, 0.0, G.LR_PSI, 0.0, eps=G.EPS_PSI)
    for t in range(c.T):
        eng.load_w(t, st["w"][t])
    nxt = torch.empty(c.B, dtype=torch.int64, device="cuda")
    eng.update(c.T - 1, *b, use_gpi=True, next_actions=nxt)
    m, _, step = eng.get_adam(c.T - 1)
    assert step == 1 and torch.equal(nxt.cpu(), info.next)
    print("| group | GPU error | float32 emulation error | max abs g | bound |")
    G.grad_close(f"{c.id} psi", G.grad_from_moments(m), g64["psi"], r32["psi"])
    G.grad_close(f"{c.id} w", G.grad_from_moments(eng.get_w(c.T - 1)[1]), g64["w"], r32["w"])
    eng.close()


# ---------------------------------------------------------------------------------------------
# look-ahead
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n_s,H", [(17, 64), (32, 64), (32, 48)])
def test_lookahead_is_bit_exact_in_both_modes(n_s, H, prec, monkeypatch):
    """tests/test_gpu_runner.py::test_lookahead_is_bit_exact at 30 steps, in fp32 and in bf16.  Where a forward from
    layer 0 computes it in-tile (the fused layer-0+1 launch: (17, 64), (32, 64)) the look-ahead's layer 0, inside the dW
    tiles, is the same fp32 product in the same order of k in both modes: everything is IDENTICAL to SFX_AHEAD=0.
    At (32, 48) the step-start layer 0 is a launch of its own that sums k in another order: both are valid fp32, the
    two runs differ at rounding level in fp32 as in bf16 (measured: heads and moments differ, no action does), and
    DESIGN.md §4 promises bit-identity for the fused geometry only.  There the runs are held to the band two Adam
    trajectories of n steps cannot leave, 2·lr·n (tests/test_gpu_bf16.py), and the difference is printed."""
    from sfx.runner import NativeEnvLoop
    from tests.test_gpu_runner import make

    spec = R.Spec(n_s, H, 7, 8, ("relu", "relu"))
    T, n = 5, 30
    out = {}
    for ahead in ("1", "0"):
        monkeypatch.setenv("SFX_AHEAD", ahead)
        eng, _ = make(spec, T, 7, max_batch=16)
        eng.set_precision(prec)
        loop = NativeEnvLoop(eng, batch=16, capacity=48, gamma=0.9, epsilon=0.2, alpha_w=0.05, episode_len=13, seed=4)
        loop.prefill(20)
        loop.set_task(1)
        loop.record(n)
        loop.run(n // 2)
        loop.run(n - n // 2)
        recs = loop.records()
        heads = torch.stack([eng.get_head(t, 0) for t in range(T)])
        targets = torch.stack([eng.get_head(t, 1) for t in range(T)])
        moms = [eng.get_adam(t) for t in range(T)]
        ws = torch.stack([eng.get_w(t)[0] for t in range(T)])
        out[ahead] = (heads, targets, moms, ws, [(r["c"], r["a_greedy"]) for r in recs], loop.action(), loop.stats())
        loop.close()
        eng.close()
    h1, t1, m1, w1, a1, f1, s1 = out["1"]
    h0, t0, m0, w0, a0, f0, s0 = out["0"]
    assert s0["ahead_pre_steps"] == 0
    # both kinds of step ran: forwarded by the step before, and (dirty minibatches, target syncs) by itself
    assert s1["ahead_pre_steps"] > 0 and s1["ahead_own_forward_steps"] > 0, s1
    assert [m[2] for m in m1] == [m[2] for m in m0]
    if not B.fused01(B.Geo(n_s, H, 7, 8)):
        dh, dt = float((h1 - h0).abs().max()), float((t1 - t0).abs().max())
        print(f"look-ahead at ({n_s}, {H}) {prec}: max |head difference| {dh:.3g}, targets {dt:.3g}; actions "
              f"{'equal' if a1 == a0 and f1 == f0 else 'differ'}")
        assert bool(torch.isfinite(h1).all()) and dh <= 2e-3 * n and dt <= 2e-3 * n
        return
    assert a1 == a0 and f1 == f0
    assert torch.equal(h1, h0) and torch.equal(t1, t0) and torch.equal(w1, w0)
    for (ma, va, sa), (mb, vb, sb) in zip(m1, m0):
        assert torch.equal(ma, mb) and torch.equal(va, vb) and sa == sb
