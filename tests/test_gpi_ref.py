"""CPU: the rule of tests/gpi_ref.py accepts a faithful float32 GPI and has teeth at the shapes of the GPU matrix.

For every case of gpi_ref.CASES the float32 CPU oracle's ψ (oracle.ref_cpu.psi_all) stands in for the kernel's.  A
numpy emulation of the GPI semantics -- one float32 fma chain per q in k order (the fma as a float64 product and
sum rounded once more to float32: the rare double rounding stays far inside the bound), exact maxima, first-index
argmaxes with -0 == +0, heads with off + t < i from the post-update ψ -- is run on
  * plain: the next actions of EVERY policy's w and the task argmax, on one set of states (what the all-task step
    and sfx_gpi compute), plus one explicit w of another scale;
  * roles: a first, a chunk-boundary and a last policy with "post" ψ from other heads, at head offsets 0 and 3;
  * ties (the cases the GPU test ties): head T-1 a copy of head 0, action A-1 a copy of action 0, and w = 0.
Then
  * the unmutated emulation is accepted everywhere;
  * at most 1 % of a case's (policy, row) argmaxes are undecided (a condition on the inputs: Case.seed);
  * each mutant is rejected on the case named in CAUGHT_AT (every case that rejects it is printed).

One mutant has no case: "-0.0 ordered below +0.0".  Every q is an fma chain that starts at +0.0, and under
round-to-nearest x + y is -0.0 only if both are, so no q, hence no maximum, is ever -0.0 short of underflow (asserted
below on every emulated q).  The rule itself rejects that order on a hand-made row, which is asserted instead.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests import gpi_ref as G

MUTANTS = ("last_index", "max_over_actions", "roles_swapped", "boundary_le", "offset_ignored", "last_head_dropped",
           "action_tail_dropped", "pair_aliases_action0", "partial_chunk_stale", "w_stride_d", "first_256_only",
           "neg_zero_below")

# the case on which the rule must reject each mutant (the branch the case was chosen for)
CAUGHT_AT = {
    "last_index": "w-vd3",            # ties
    "max_over_actions": "w-edge",
    "roles_swapped": "w-full",
    "boundary_le": "w-vd4",
    "offset_ignored": "w-vd3",
    "last_head_dropped": "w-vd1",     # T = 9: chunks 8 + 1, 55 idle lanes
    "action_tail_dropped": "w-full",  # A = 17: a third a0 pass for action 16
    "pair_aliases_action0": "w-vd3",  # A = 9: a0 = 8 pairs with 12
    "partial_chunk_stale": "w-vd4",   # T = 52: chunks 6·8 + 4
    "w_stride_d": "n-odd-d",          # d = 6, dpad = 8
    "first_256_only": "n-odd-d",      # T·A = 280, narrow, two passes
}


def chain32(psi: np.ndarray, w: np.ndarray) -> np.ndarray:
    q = np.zeros(psi.shape[:-1], dtype=np.float32)
    for k in range(psi.shape[-1]):
        q = (psi[..., k].astype(np.float64) * np.float64(w[k]) + q.astype(np.float64)).astype(np.float32)
    return q


def first_argmax(m: np.ndarray, mut=None) -> np.ndarray:
    """First argmax over the last axis of float32 values, -0 == +0."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    if mut == "neg_zero_below":  # ordered by the sign-magnitude bits
        u = m.view(np.uint32)
        key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
        return np.argmax(key, axis=-1)
    if mut == "last_index":
        return m.shape[-1] - 1 - np.argmax(m[..., ::-1], axis=-1)
    return np.argmax(m, axis=-1)


def emulate(psi, W, i, post=None, off=0, mut=None, w=None):
    """GPI of policy i (reward row W[i], or w) on float32 ψ [B, T, A, d] -> dict(q, next, task)."""
    B, T, A, d = psi.shape
    if w is None:
        if mut == "w_stride_d" and d % 4:
            dpad = (d + 3) // 4 * 4
            Wp = np.zeros((W.shape[0], dpad), dtype=np.float32)
            Wp[:, :d] = W
            w = Wp.reshape(-1)[i * d:i * d + d]
        else:
            w = W[i]
    if post is not None:
        t = np.arange(T)
        before = {"boundary_le": off + t <= i, "offset_ignored": t < i}.get(mut, off + t < i)
        if mut == "roles_swapped":
            before = ~before
        psi = np.where(before[None, :, None, None], post, psi)
    q = chain32(psi, w)
    qa = q.copy()  # what enters the maxima over heads
    if mut == "last_head_dropped" and T % 64:
        qa[:, T - 1] = -np.inf
    if mut == "first_256_only":
        qa.reshape(B, T * A)[:, 256:] = -np.inf
    m_a, m_t = qa.max(axis=1), q.max(axis=2)
    if mut == "action_tail_dropped":
        m_a[:, 8 * (A // 8):] = -np.inf
    if mut == "pair_aliases_action0":  # wave w: a0 = w, w + 8, ...; the pair a0 + 4 >= A lands on (a0 + 4) % A
        for a0 in range(A):
            if a0 % 8 < 4 and a0 + 4 >= A:
                m_a[:, (a0 + 4) % A] = m_a[:, 0]
    nxt = first_argmax(m_t if mut == "max_over_actions" else m_a, mut)
    return dict(q=q, next=nxt, task=first_argmax(m_t, mut), m_a=m_a)


def policies_of(T: int):
    return sorted({0, 8 * ((T - 1) // 8), T - 1})


@functools.lru_cache(maxsize=None)
def inputs(cid: str):
    """The float32 ψ tables of one case: plain, post (other heads), tied."""
    c = G.case(cid)
    spec = G.spec_of(c)
    online, w, S, S1, w_x = G.problem(c)
    from sfx.init import reference_heads

    other, _ = reference_heads(c.T, G.N_S, G.H, c.A, c.d, G.ACTS, seed=c.seed + 50)
    out = dict(c=c, W=w.numpy(), w_x=w_x.numpy(), psi=R.psi_all(online, spec, S).numpy(),
               pre=R.psi_all(online, spec, S1).numpy(), post=R.psi_all(other, spec, S1).numpy())
    if c.ties:
        out["tied"] = R.psi_all(G.tie_heads(online, c, *G.tie_indices(c)), spec, S).numpy()
    return out


def evaluate(cid: str, mut=None):
    """Run the emulation over the case's evaluations -> (rejections, undecided, argmaxes).  A rejection is a
    string naming the evaluation whose q or index the rule refuses."""
    x = inputs(cid)
    c, W = x["c"], x["W"]
    bad, und, tot = [], 0, 0

    def idx(what, got, m64, Bm, count=True):
        nonlocal und, tot
        ok, dec = G.judge(got, m64, Bm)
        if count:
            und += int((~dec).sum())
            tot += dec.size
        if not ok.all():
            bad.append(what)

    def one(what, psi, i, w=None, post=None, off=0, count=False, Wt=W):
        e = emulate(psi, Wt, i, post, off, mut, w)
        assert not np.signbit(e["q"][e["q"] == 0]).any(), "an fma chain from +0.0 gave -0.0"
        ref = G.reference(psi, Wt[i] if w is None else w, post, i, off)
        if (np.abs(e["q"].astype(np.float64) - ref.q64) > ref.bound).any():
            bad.append(what + " q")
        idx(what + " next", e["next"], ref.m_a, ref.B_a, count)
        return e, ref

    # plain: every policy's next actions (stale results of a partial last chunk: the chunked kernels' mutant)
    nxt = []
    for i in range(c.T):
        nxt.append(one(f"plain i={i}", x["psi"], i, count=True))
    if mut == "partial_chunk_stale" and c.T % 8 and c.T > 8:
        i0 = 8 * (c.T // 8)
        for i in range(i0, c.T):
            idx(f"plain i={i} next (stale)", nxt[i0 - 1][0]["next"], nxt[i][1].m_a, nxt[i][1].B_a, False)
    for i in (0, c.T - 1):
        e, ref = nxt[i]
        idx(f"plain i={i} task", e["task"], ref.m_t, ref.B_t)
    e, ref = one("explicit w", x["psi"], 0, w=x["w_x"], count=True)
    idx("explicit w task", e["task"], ref.m_t, ref.B_t)
    # roles
    for off in (0, 3):
        Wt = np.concatenate([W, W[::-1], W])[:c.T + off]  # the global reward table of a sharded handle
        for i in policies_of(c.T):
            one(f"roles off={off} i={i + off}", x["pre"], i + off, post=x["post"], off=off, Wt=Wt)
    # ties
    if c.ties:
        for i in (0, c.T - 1):
            e, ref = one(f"ties i={i}", x["tied"], i)
            idx(f"ties i={i} task", e["task"], ref.m_t, ref.B_t, False)
        z = np.zeros(c.d, dtype=np.float32)
        e, ref = one("ties w=0", x["tied"], 0, w=z)
        idx("ties w=0 task", e["task"], ref.m_t, ref.B_t, False)
        assert mut is not None or (not e["next"].any() and not e["task"].any())
    return bad, und, tot


@pytest.mark.parametrize("cid", [c.id for c in G.CASES])
def test_reference_accepts_the_emulation_and_the_cap_holds(cid):
    bad, und, tot = evaluate(cid)
    print(f"{cid}: {und} of {tot} argmaxes undecided")
    assert not bad, bad
    assert und <= 0.01 * tot, f"{cid}: {und} of {tot} argmaxes undecided: more than 1 %"


@pytest.mark.parametrize("mut", [m for m in MUTANTS if m in CAUGHT_AT])
def test_mutant_is_rejected_at_its_case(mut):
    catching = [c.id for c in G.CASES if evaluate(c.id, mut)[0]]
    print(f"mutant {mut}: rejected on {catching}")
    bad = evaluate(CAUGHT_AT[mut], mut)[0]
    assert bad, f"mutant {mut} passes on {CAUGHT_AT[mut]}"
    print(f"mutant {mut} at {CAUGHT_AT[mut]}: {bad[:4]}")


def test_neg_zero_order_is_rejected_by_the_rule():
    m = np.array([[-0.0, 0.0, -1.0]], dtype=np.float32)
    assert first_argmax(m)[0] == 0 and first_argmax(m, "neg_zero_below")[0] == 1
    z = np.zeros_like(m, dtype=np.float64)
    ok, dec = G.judge(first_argmax(m, "neg_zero_below"), m.astype(np.float64), z)
    assert not ok[0] and not dec[0]
    ok, _ = G.judge(first_argmax(m), m.astype(np.float64), z)
    assert ok[0]


def test_judge_by_hand():
    m = np.array([[1.0, 3.0, 2.9, 3.0]])
    B = np.full_like(m, 0.04)
    assert G.judge([1], m, B)[0][0] and not G.judge([3], m, B)[0][0]      # equal values: the first one only
    assert not G.judge([2], m, B)[0][0] and G.judge([2], m, B + 0.01)[0][0]  # 0.1 <= 2 * 0.05
    assert not G.judge([0], m, B + 0.01)[0][0] and not G.judge([4], m, B)[0][0] and not G.judge([-1], m, B)[0][0]
    assert not G.judge([1], m, B)[1][0]                                      # a tie is never decided
    assert G.judge([1], np.array([[1.0, 3.0, 2.9]]), np.full((1, 3), 0.04))[1][0]
    assert G.gamma(8) == 8 * 2.0 ** -24 / (1 - 8 * 2.0 ** -24)


def test_reference_by_hand():
    psi = np.array([[[[1.0, 2.0], [3.0, -4.0]], [[0.5, 0.5], [-1.0, 1.0]]]], dtype=np.float32)  # [1, 2, 2, 2]
    post = -psi
    w = np.array([2.0, 1.0], dtype=np.float32)
    r = G.reference(psi, w)
    assert r.q64.tolist() == [[[4.0, 2.0], [1.5, -1.0]]] and (r.next, r.task) == (0, 0)
    assert np.allclose(r.bound, G.gamma(2) * np.array([[[4.0, 10.0], [1.5, 3.0]]]), rtol=1e-15)
    assert r.B_a.tolist() == r.bound.max(axis=1).tolist() and r.B_t.tolist() == r.bound.max(axis=2).tolist()
    assert r.selection(0, 1, True) == (0, 0) and r.selection(0, 1, False) == (1, 0)
    # head 0 from post for policy 1 at offset 0; no head from post at offset 0 for policy 0; offset 1: none for 1
    assert G.reference(psi, w, post, 1, 0).q64.tolist() == [[[-4.0, -2.0], [1.5, -1.0]]]
    assert G.reference(psi, w, post, 0, 0).q64.tolist() == r.q64.tolist()
    assert G.reference(psi, w, post, 1, 1).q64.tolist() == r.q64.tolist()
    assert G.reference(psi, w, post, 3, 1).q64.tolist() == (-r.q64).tolist()
    with pytest.raises(AssertionError):
        G.reference(psi.astype(np.float64), w)
