"""Float64 reference of generalised policy improvement (GPI) with a derived error bound, the rule by which an
index returned by a float32 kernel is accepted, and the shapes of tests/test_gpu_gpi_matrix.py.

GPI: q[b, t, a] = ψ_t(s_b)[a]·w, m_a = max_t q, m_t = max_a q, next = first argmax_a m_a, task = first argmax_t m_t,
selection = (c, first argmax_a q[c]) with c = task (GPI) or the active task (features/successor.py:223-246,
features/deep.py:101-103, agents/sfdqn.py:39-45).  Heads may come from two states: head t enters policy i's GPI
from the "post" ψ if off + t < i and from the "pre" ψ otherwise (k_tdg, wide_maxima, k_qmax; agents/sfdqn.py:57-60).

Bound.  Every GPI kernel forms q by one fmaf chain over k = 0 .. d-1 from float32 inputs.  For such a chain
(Higham, Accuracy and Stability of Numerical Algorithms, §3.1 with one rounding per step)
    |q - Σ_k ψ_k w_k| <= γ_d Σ_k |ψ_k| |w_k|,   γ_d = d u / (1 - d u),   u = 2^-24,
provided the ψ are the float32 values the kernel itself read (and nothing underflows).  max is exact, so
B_a = max_t bound bounds the error of m_a and B_t = max_a bound that of m_t.

Rule.  q: every entry within its bound.  An index j* returned for an argmax over m: the kernel's value at j* is
at least its value at the float64 argmax, each within max(B) of the float64 value, so
m64[j*] >= max(m64) - 2 max(B) must hold; a float64 top-2 gap above 2 max(B) therefore forces j* = argmax64 (the
row is "decided"), any other row is "undecided" and still checked by the inequality.  Exactly equal float64
values come from exactly equal float32 inputs (copied heads or actions, w = 0), where the kernels' values are
equal too and the first-index rule of torch.argmax applies: j* must be the smallest index among them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

U = 2.0 ** -24
N_S, H, ACTS = 17, 16, ("relu", "relu")


def gamma(d: int) -> float:
    return d * U / (1.0 - d * U)


@dataclass(frozen=True)
class Case:
    """One shape of the matrix.  seed: reference_heads' seed and, + 100, the states' generator (chosen so that the
    case meets the cap of test_gpi_ref.py).  step: (head seed, step seed, gap) of the all-task steps of
    test_gpu_gpi_matrix.py, gap = the smallest float64 top-2 gap / max |q| over every in-order next-action and
    selection argmax of those steps (>= 1e-4, tests/adam_ref.py's margin); None: T < 5, no all-task part."""
    id: str
    T: int
    A: int
    d: int
    B: int = 16
    seed: int = 0
    step: Optional[tuple] = None
    ties: bool = False
    branch: str = ""


CASES = (
    Case("w-vd1", 9, 32, 4, step=(0, 6, 1.45e-04), branch="wide VD=1, four full a0 passes, 55 lanes idle, chunks 8 + 1"),
    Case("w-vd3", 33, 9, 12, step=(0, 8, 2.69e-04), ties=True,
         branch="wide VD=3, second a0 pass for wave 0 only, pair out of range, chunks 4·8 + 1"),
    Case("w-vd4", 52, 5, 16, step=(2, 39, 1.28e-04), branch="wide VD=4, T·A = 260, pair valid for wave 0 only, chunks 6·8 + 4"),
    Case("w-full", 64, 17, 8, step=(5, 30, 1.01e-04), ties=True, branch="wide, all lanes live, three a0 passes, A·d = 136"),
    Case("w-edge", 37, 7, 8, step=(0, 22, 1.24e-04), branch="T·A = 259, the first wide shape"),
    Case("n-edge", 32, 8, 8, step=(0, 7, 1.96e-04), branch="T·A = 256, narrow, every thread of the fast bodies live"),
    Case("n-odd-d", 40, 7, 6, step=(0, 15, 1.45e-04), ties=True, branch="narrow scalar loops, two passes, dpad != d"),
    Case("n-a33", 8, 33, 4, step=(0, 6, 3.46e-04), branch="A > 32 forces narrow; qdots_vec<2,8>, 128-thread k_sel1m"),
    Case("n-d20", 20, 14, 20, step=(0, 6, 1.09e-04), branch="d > 16 forces narrow scalar loops at d % 4 == 0"),
    # step seed 5 (gap 4.74e-4) left every round-0 speculation standing at T = 6; with 6 policy 4's fails in step 1
    Case("n-d12", 6, 9, 12, step=(0, 6, 5.31e-04), branch="qdots_vec<4,4>; rows = 4, fast bodies at V4 = 3"),
    Case("rows-tail", 5, 17, 4, B=32, step=(0, 5, 1.24e-03), branch="rows = 3, n = 255, last workgroup nb = 2"),
    Case("a-max", 2, 256, 1, ties=True, branch="the action limit; 256-thread k_sel1m<1>, s_ma full"),
)


def case(cid: str) -> Case:
    return next(c for c in CASES if c.id == cid)


def spec_of(c: Case):
    from oracle import ref_cpu as R

    return R.Spec(N_S, H, c.A, c.d, ACTS)


def problem(c: Case):
    """(online [T, P], w [T, d], S [B, n_s], S1 [B, n_s], w_x [d]): the heads of sfx.init.reference_heads, two sets of
    states and one explicit reward vector (larger than the U(-0.01, 0.01) rows: another scale of q)."""
    from sfx.init import reference_heads

    online, w = reference_heads(c.T, N_S, H, c.A, c.d, ACTS, seed=c.seed)
    gen = torch.Generator().manual_seed(100 + c.seed)
    S, S1 = torch.randn(c.B, N_S, generator=gen), torch.randn(c.B, N_S, generator=gen)
    w_x = torch.randn(c.d, generator=gen)
    return online, w, S, S1, w_x


def tie_heads(online: torch.Tensor, c: Case, t1: int, t2: int, a1: int, a2: int) -> torch.Tensor:
    """Head t2 a copy of head t1 and, in every head, the output-layer rows and bias of action a2 copies of a1's."""
    from oracle import ref_cpu as R

    assert t1 < t2 < c.T and a1 < a2 < c.A
    out = online.clone()
    for t in range(c.T):
        W, b = R.unpack(out[t], spec_of(c))[-1]
        W[a2 * c.d:(a2 + 1) * c.d] = W[a1 * c.d:(a1 + 1) * c.d]
        b[a2 * c.d:(a2 + 1) * c.d] = b[a1 * c.d:(a1 + 1) * c.d]
    out[t2] = out[t1]
    return out


def tie_indices(c: Case):
    """(t1, t2, a1, a2): copies across the 64-lane / 8-policy chunk and action-pass boundaries where the shape has them."""
    return 0, c.T - 1, 0, c.A - 1


def forward64(online: torch.Tensor, c: Case, S: torch.Tensor) -> np.ndarray:
    """ψ [B, T, A, d] of the loaded float32 parameters and states, evaluated in float64."""
    from oracle import ref_cpu as R

    return R.psi_all(online.double(), spec_of(c), S.double()).numpy()


@dataclass
class Ref:
    q64: np.ndarray    # [B, T, A]
    bound: np.ndarray  # [B, T, A]
    m_a: np.ndarray    # [B, A]   max over heads
    m_t: np.ndarray    # [B, T]   max over actions
    B_a: np.ndarray    # [B, A]
    B_t: np.ndarray    # [B, T]
    next: np.ndarray   # [B] first argmax_a m_a
    task: np.ndarray   # [B] first argmax_t m_t

    def selection(self, b: int, task_index: int, use_gpi: bool):
        c = int(self.task[b]) if use_gpi else task_index
        return c, int(np.argmax(self.q64[b, c]))


def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def reference(psi, w, post=None, i: Optional[int] = None, off: int = 0) -> Ref:
    """psi [B, T, A, d], w [d] (float32 values as the kernel read them).  post, i, off: head t from `post` where
    off + t < i, from `psi` otherwise."""
    psi, w = _np(psi), _np(w).reshape(-1)
    assert psi.dtype == np.float32 and w.dtype == np.float32, "the bound holds for the kernel's own float32 inputs"
    if post is not None:
        post = _np(post)
        assert post.dtype == np.float32 and post.shape == psi.shape
        before = off + np.arange(psi.shape[1]) < i
        psi = np.where(before[None, :, None, None], post, psi)
    p64, w64 = psi.astype(np.float64), w.astype(np.float64)
    q64 = p64 @ w64
    bound = gamma(psi.shape[-1]) * (np.abs(p64) @ np.abs(w64))
    m_a, m_t = q64.max(axis=1), q64.max(axis=2)
    return Ref(q64, bound, m_a, m_t, bound.max(axis=1), bound.max(axis=2), np.argmax(m_a, axis=1),
               np.argmax(m_t, axis=1))


def judge(idx, m64: np.ndarray, Bm: np.ndarray):
    """Rows of values m64 [R, n] with bounds Bm [R, n] and the returned indices idx [R] -> (ok [R], decided [R])."""
    idx = _np(idx).astype(np.int64).reshape(-1)
    m64, Bm = np.atleast_2d(m64), np.atleast_2d(Bm)
    R, n = m64.shape
    assert idx.shape == (R,) and Bm.shape == m64.shape
    tol = 2.0 * Bm.max(axis=1)
    top = m64.max(axis=1)
    inr = (idx >= 0) & (idx < n)
    val = m64[np.arange(R), np.where(inr, idx, 0)]
    ok = inr & (val >= top - tol)
    earlier = (np.arange(n)[None, :] < idx[:, None]) & (m64 == val[:, None])  # an equal value at a smaller index
    ok &= ~earlier.any(axis=1)
    if n > 1:
        s = np.sort(m64, axis=1)
        decided = s[:, -1] - s[:, -2] > tol
    else:
        decided = np.ones(R, dtype=bool)
    return ok, decided


@dataclass
class Tally:
    """What one case's table row reports."""
    worst_q: float = 0.0
    decided: int = 0
    undecided: int = 0
    e_psi: float = 0.0

    def row(self, cid: str) -> str:
        return f"| {cid} | {self.worst_q:.3f} | {self.decided} | {self.undecided} | {self.e_psi:.2e} |"


HEADER = "| case | worst abs(q - q64) / bound | decided | undecided | e_psi |\n|---|---|---|---|---|"


def check_q(q, ref: Ref, what: str, tally: Optional[Tally] = None) -> float:
    q = _np(q).astype(np.float64).reshape(ref.q64.shape)
    err = np.abs(q - ref.q64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / ref.bound)
    worst = float(ratio.max())
    if tally is not None:
        tally.worst_q = max(tally.worst_q, worst)
    assert worst <= 1.0, f"{what}: |q - q64| = {worst:.3g} x the bound at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


def check_index(idx, m64, Bm, what: str, tally: Optional[Tally] = None):
    ok, decided = judge(idx, m64, Bm)
    if tally is not None:
        tally.decided += int(decided.sum())
        tally.undecided += int((~decided).sum())
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"{what}: rows {bad[:8].tolist()} returned {_np(idx).reshape(-1)[bad[:8]].tolist()}, float64 "
                           f"argmax {np.argmax(np.atleast_2d(m64), axis=1)[bad[:8]].tolist()}")
    return decided


def check_next(nxt, ref: Ref, what: str, tally=None):
    return check_index(nxt, ref.m_a, ref.B_a, what + " next", tally)


def check_task(task, ref: Ref, what: str, tally=None):
    return check_index(task, ref.m_t, ref.B_t, what + " task", tally)


def check_selection(c_a, ref: Ref, rows, task_index: int, use_gpi: bool, what: str, tally=None):
    """(c, a) per row of `rows`: c by the rule over m_t (GPI) or the active task; a by the rule over q[c] for the
    c that was returned."""
    c_a = _np(c_a).reshape(-1, 2)
    rows = np.asarray(rows).reshape(-1)
    if use_gpi:
        check_index(c_a[:, 0], ref.m_t[rows], ref.B_t[rows], what + " selected task", tally)
    else:
        assert (c_a[:, 0] == task_index).all(), f"{what}: selected task {c_a[:, 0].tolist()} is not the active one"
    c = c_a[:, 0]
    check_index(c_a[:, 1], ref.q64[rows, c], ref.bound[rows, c], what + " selected action", tally)
