"""GPU: every GPI kernel variant at the edges of its dispatch, against the float64 reference of tests/gpi_ref.py.

The host picks one of about a dozen GPI implementations from (T, A, d, M): gpi_row's two bodies, k_sel1m<1|2|4>,
k_tdg's strided loop, ver_block's row packing with its two bodies, and the wide kernels k_tdgw / k_verw<VD> past
T·A = 256 (sfx_gpiw.h).  gpi_ref.CASES holds, per branch, the smallest shape that still reaches it (Case.branch);
tests/test_gpi_ref.py shows on the CPU that mutants of exactly those branches are rejected at those shapes.

Nothing is compared with the code under test: q, task, next and the selections are judged by gpi_ref's rule from
the ψ the library itself returned (the float32 values its GPI kernels read), and that ψ against a float64 forward
of the loaded parameters.  The only equalities are between two library paths that promise the same bits.

sfx_update's next actions against sfx_gpi's, read off run_fwd: at H = 16 every layer of the heads has K = 17 or
K = 16, never a multiple of 32, so each forward launch of either entry point is k_fwd<false, false> with one
column tile per workgroup, no tail rows, no GEMV (N < 512) and no fused layer-0+1 launch (K_1 % 32 != 0).  In that
kernel an output element's accumulation order depends on K and on the element's place in its 32-row tile only;
both calls forward the same B rows from row 0.  So the R_S1 block of sfx_update and the R_G block of sfx_gpi hold
the same bits and the next actions must be equal, which is asserted on top of the rule.

Each case prints one row of the table kept in profiles/gpi_matrix.md.
"""
import numpy as np
import pytest
import torch

from tests import gpi_ref as G
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def engine(c, online, w, lr=0.0):
    from sfx.engine import SFEngine

    eng = SFEngine(c.T, G.N_S, G.H, c.A, c.d, G.ACTS, max_batch=32)
    eng.set_adam(lr, 0.0, lr, 0.0)
    load(eng, online, w)
    return eng


def load(eng, online, w):
    for t in range(eng.T):
        eng.load_head(t, online[t], 0)
        eng.load_head(t, online[t], 1)
        eng.load_w(t, w[t])


def w_stride_of(c) -> int:
    """Row stride of test_actions' W: past d on the d % 4 == 0 cases (rows stay 16-byte aligned), d + 1 on n-edge
    (T·A = 256, d = 8: gpi_row's fast body but for the alignment of three rows in four), d elsewhere."""
    return c.d + 1 if c.id == "n-edge" else c.d + 4 if c.d % 4 == 0 else c.d


def strided_test_actions(eng, S, W, stride):
    """sfx_test_actions with rows of W `stride` floats apart -> (q [E, T, A], (c, a) [E, 2])."""
    from sfx._lib import check, lib

    E = S.shape[0]
    buf = torch.zeros(E, stride, device="cuda")
    buf[:, :eng.d] = W.cuda()
    Sd = S.cuda().contiguous()
    q = torch.empty(E, eng.T, eng.A, device="cuda")
    out = torch.empty(E, 2, dtype=torch.long, device="cuda")
    check(lib.sfx_test_actions(eng._h, Sd.data_ptr(), E, buf.data_ptr(), stride, q.data_ptr(), out.data_ptr()),
          "sfx_test_actions")
    torch.cuda.synchronize()
    return q, out.cpu()


def batch_of(c, S, S1, seed=7):
    gen = torch.Generator().manual_seed(seed)
    B = S.shape[0]
    a = torch.randint(0, c.A, (B,), generator=gen)
    phi = torch.rand(B, c.d, generator=gen)
    gamma = torch.where(torch.rand(B, generator=gen) < 0.1, 0.0, 0.9)
    return a, phi, gamma


def policies_of(T):
    return sorted({0, 8 * ((T - 1) // 8), T - 1})


@pytest.mark.parametrize("cid", [c.id for c in G.CASES])
def test_gpi_case(cid):
    c = G.case(cid)
    online, w, S, S1, w_x = G.problem(c)
    eng = engine(c, online, w)
    tally = G.Tally()
    psi64 = {1: G.forward64(online, c, S[:1]), c.B: G.forward64(online, c, S)}

    # a. sfx_gpi at B rows and at one row; w of a first and a last head and an explicit one
    keep = {}
    for rows in (c.B, 1):
        for name, kw, wv in (("w0", dict(w_index=0), w[0]), ("wT", dict(w_index=c.T - 1), w[c.T - 1]),
                             ("wx", dict(w=w_x), w_x)):
            psi, q, task, nxt = eng.gpi(S[:rows], want_psi=True, **kw)
            psi = psi.cpu()
            what = f"{cid} sfx_gpi rows={rows} {name}"
            np.testing.assert_allclose(psi.numpy(), psi64[rows], rtol=1e-4, atol=1e-6, err_msg=what)
            tally.e_psi = max(tally.e_psi, float(np.abs(psi.numpy() - psi64[rows]).max()))
            ref = G.reference(psi, wv)
            G.check_q(q, ref, what, tally)
            G.check_task(task, ref, what, tally)
            G.check_next(nxt, ref, what, tally)
            keep[rows, name] = (psi, q.clone(), ref)

    # b. select_action: the same bits as sfx_gpi on the row, (c, a) by the rule
    for task_index, name in ((0, "w0"), (c.T - 1, "wT")):
        psi, q1, ref = keep[1, name]
        for use_gpi in (True, False):
            q_out = torch.empty(1, c.T, c.A, device="cuda")
            sel = eng.select_action(S[0], task_index, use_gpi, q_out).cpu()
            what = f"{cid} select_action task={task_index} gpi={use_gpi}"
            assert torch.equal(q_out, q1), what + ": q differs from sfx_gpi's"
            G.check_selection(sel, ref, [0], task_index, use_gpi, what, tally)
    # test_actions: per-row reward weights, strided
    gen = torch.Generator().manual_seed(11)
    W = (torch.randn(c.B, c.d, generator=gen) * 0.01).contiguous()
    q_rows, sel = strided_test_actions(eng, S, W, w_stride_of(c))
    psi_rows = keep[c.B, "w0"][0]
    w_dev = torch.empty(c.d, device="cuda")
    for e in range(c.B):
        w_dev.copy_(W[e])
        _, q, _, _ = eng.gpi(S, w=w_dev)
        what = f"{cid} test_actions row {e}"
        assert torch.equal(q_rows[e], q[e]), what + ": q differs from sfx_gpi's"
        G.check_selection(sel[e], G.reference(psi_rows[e:e + 1], W[e]), [0], 0, True, what, tally)

    # c. update(i, use_gpi=True): next actions by the rule, and sfx_gpi's bit for bit (module docstring)
    a, phi, gamma = batch_of(c, S, S1)
    for i in policies_of(c.T):
        psi1, _, _, nxt_gpi = eng.gpi(S1, w_index=i, want_psi=True)
        nxt = torch.full((c.B,), -1, dtype=torch.long, device="cuda")
        eng.update(i, S, a, None, phi, S1, gamma, use_gpi=True, next_actions=nxt)
        what = f"{cid} update i={i}"
        G.check_next(nxt, G.reference(psi1.cpu(), w[i]), what, tally)
        assert torch.equal(nxt, nxt_gpi), what + ": next actions differ from sfx_gpi's"

    # d. round 0 of the all-task step: every policy's next actions from the pre-step heads
    if c.step is not None:
        psi1 = eng.gpi(S1, w_index=0, want_psi=True)[0].cpu()
        eng.set_spec_rounds(1)
        eng.update_all(S, a, phi, S1, gamma)
        spec_next = eng.debug_spec_next(c.B)[0]
        eng.settle()
        for i in range(c.T):
            G.check_next(spec_next[i], G.reference(psi1, w[i]), f"{cid} all-task round 0 policy {i}", tally)

    print("\n" + G.HEADER + "\n" + tally.row(cid))
    eng.close()


@pytest.mark.parametrize("mode", ["two-rounds", "host-rounds", "one-round"])
@pytest.mark.parametrize("cid", [c.id for c in G.CASES if c.step is not None])
def test_all_task_steps_match_in_order_oracle(cid, mode):
    """Two all-task steps against the in-order oracle (tests/test_gpu_step.run_steps): k_ver / k_verw must flag every
    policy whose speculated next actions the earlier heads' updates changed, or the parameters differ.  Seeds from
    Case.step: every in-order argmax has a float64 top-2 gap >= 1e-4 of max |q|.

    two-rounds: the default two device rounds, unforced.  host-rounds: every step's device rounds treated as failed
    from policy 1 (sfx_debug_force_rerun).  one-round: one device round, unforced -- step_finish's `first` is the
    verdict of the LAST device round, and at two rounds the second round repaired all 22 steps of these cases on the
    GPU (first == T throughout), so that the verifier has met a real mismatch is asserted here, where the verdict is
    round 0's: at least one step per case has first < T and is finished by host rounds from there."""
    from tests.test_gpu_step import run_steps, setup

    c = G.case(cid)
    head_seed, step_seed, gap = c.step
    assert gap >= 1e-4
    spec = G.spec_of(c)
    eng, st = setup(spec, c.T, seed=head_seed)
    if mode == "one-round":
        eng.set_spec_rounds(1)
    eng.debug_force_rerun(1 if mode == "host-rounds" else -1)
    k = 2
    agree = run_steps(eng, st, spec, c.T, k=k, seed=step_seed)
    print(f"{cid} {mode}: first == T in {agree} of {k} steps")
    if mode == "one-round":
        assert agree < k, f"{cid}: round 0's speculation held in every step: the verifier never met a mismatch"
    eng.close()


@pytest.mark.parametrize("cid", [c.id for c in G.CASES if c.ties])
def test_exact_ties_take_the_first_index(cid):
    """Head t2 a copy of head t1 < t2, action a2 a copy of a1 < a2 in every head: no path returns t2 or a2; with
    w = 0 every q is +0 and every index 0."""
    c = G.case(cid)
    online, w, S, S1, w_x = G.problem(c)
    t1, t2, a1, a2 = G.tie_indices(c)
    eng = engine(c, G.tie_heads(online, c, t1, t2, a1, a2), w)
    a, phi, gamma = batch_of(c, S, S1)
    gen = torch.Generator().manual_seed(13)
    W = (torch.randn(c.B, c.d, generator=gen) * 0.01).contiguous()

    def paths(ws, tag):
        out = []  # (what, tasks or None, actions)
        for i in (0, c.T - 1):
            psi, q, task, nxt = eng.gpi(S, w_index=i, want_psi=True)
            ref = G.reference(psi.cpu(), ws[i])
            G.check_task(task, ref, f"{cid} {tag} sfx_gpi w{i}")
            G.check_next(nxt, ref, f"{cid} {tag} sfx_gpi w{i}")
            out.append((f"sfx_gpi w{i}", task.cpu(), nxt.cpu()))
            for use_gpi in (True, False):
                sel = eng.select_action(S[0], 0, use_gpi).cpu()
                out.append((f"select_action gpi={use_gpi}", sel[:1], sel[1:]))
            nx = torch.full((c.B,), -1, dtype=torch.long, device="cuda")
            eng.update(i, S, a, None, phi, S1, gamma, use_gpi=True, next_actions=nx)
            out.append((f"update i={i}", None, nx.cpu()))
        return out

    for what, tasks, acts in paths(w, "ties"):
        assert tasks is None or not (tasks == t2).any(), f"{cid} {what}: returned the copied head {t2}"
        assert not (acts == a2).any(), f"{cid} {what}: returned the copied action {a2}"
    _, sel = strided_test_actions(eng, S, W, w_stride_of(c))
    assert not (sel[:, 0] == t2).any() and not (sel[:, 1] == a2).any(), f"{cid} test_actions: a copy was returned"

    zero = torch.zeros_like(w)
    for t in range(c.T):
        eng.load_w(t, zero[t])
    for what, tasks, acts in paths(zero, "w=0"):
        assert tasks is None or not tasks.any(), f"{cid} w=0 {what}: task {tasks.tolist()}"
        assert not acts.any(), f"{cid} w=0 {what}: action {acts.tolist()}"
    _, _, task, nxt = eng.gpi(S, w=torch.zeros(c.d))
    assert not task.any() and not nxt.any()
    _, sel = strided_test_actions(eng, S, torch.zeros(c.B, c.d), w_stride_of(c))
    assert not sel.any(), f"{cid} w=0 test_actions: {sel.tolist()}"
    eng.close()
