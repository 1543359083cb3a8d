"""The Adam step in exact arithmetic, its float32 error bound, and the mutants the bound has to catch.

Shared by tests/test_adam_ref.py (CPU: the float32 oracle meets the bound, every mutant leaves it) and
tests/test_gpu_adam.py (GPU: every update path's epilogue against the same bound).

Expected values.  The kernel's promise (AdamHP / adam_consts / adam_apply in csrc/sfx_kernels.h) is torch's
single-tensor Adam with its constants narrowed to float32 where ATen narrows them:

    omb1 = f32(1 - b1)   b2 = f32(b2)   omb2 = f32(1 - b2)   eps = f32(eps)   wd = f32(wd)
    bc1 = 1 - b1^k, bc2 = 1 - b2^k in double;   bc2s = f32(sqrt(bc2))   nss = f32(-(lr / bc1))

    G = g + wd p        M = m0 + omb1 (G - m0)        V = b2 v0 + omb2 G^2
    D = sqrt(V) / bc2s + eps        Q = nss M / D        P = p + Q

expect() evaluates that in float64 on the float32 inputs (p, g, m0, v0): the exact-arithmetic statement.

Bound.  u = 2^-24 is the float32 unit roundoff; every float32 operation (add, multiply, fma, divide, square root:
all correctly rounded) returns its exact result times (1 + e), |e| <= u.  Count the roundings on each output's
path and multiply each by the magnitude of the value it rounds, never by the output itself (G - m0 cancels):

    e_G  (decay on)    fl(wd p): u |wd p|;  the sum: u (|g| + |wd p|)          e_G = u (|g| + 2 |wd p|), 0 if wd = 0
    m'                 e_G arrives times omb1;  fl(G - m0): u (|G| + |m0|), times omb1;
                       the fma's one rounding: u |M| <= u (|m0| + omb1 (|G| + |m0|))
                       b_m = omb1 e_G + u (|m0| + 2 omb1 (|G| + |m0|))
    v'                 e_G arrives as 2 omb2 |G| e_G;  fl(v0 b2): u b2 v0;  fl(omb2 G), fl(. G): 2 u omb2 G^2;
                       the sum: u (b2 v0 + omb2 G^2)
                       b_v = 2 omb2 |G| e_G + u (2 b2 v0 + 3 omb2 G^2)
    D                  sqrt carries b_v as b_v / (2 sqrt V) and rounds: u sqrt V;  the division by bc2s rounds:
                       u sqrt V / bc2s;  the sum with eps: u D
                       e_D = (b_v / (2 sqrt V) + 2 u sqrt V) / bc2s + u D
    p'                 the quotient: M's error |nss| b_m / D, D's error |Q| e_D / D, fl(nss m') and the division
                       2 u |Q|;  the final sum rounds to half an ulp of p': u |P|
                       b_p = u |P| + |nss| b_m / D + |Q| (e_D / D + 2 u)

A library that spends one rounding more on the lerp (start + w (end - start) without the fma: one more
u omb1 (|G| + |m0|)) or orders v's product the other way stays inside these counts, which is why torch's own CPU
kernels (oracle.ref_cpu.adam_ in float32) are held to the same bound in tests/test_adam_ref.py.  The bounds are
first order in u; GUARD = 1 + 2^-10 covers the second-order terms (relative errors here are below 16 u, so the
products of two of them are below 2^-40 of a bound) and the last-bit freedom of a double-precision pow.  Where a
bound is exactly 0 (G = m0 = 0: a dead unit's weights at step 1 without decay) the output must be exactly
expected.  No number here is fitted to what a GPU returned.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import ref_cpu as R

U = 2.0 ** -24
GUARD = 1.0 + 2.0 ** -10


# ---------------------------------------------------------------------------------------------
# hyper-parameters
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HP:
    """One set of optimizer knobs.  Within a non-default set every value differs from every other, so a group
    that reads another group's constants cannot pass.  The decays are sized so that wd p is comparable to g on the
    problems of tests/grad_ref.py (ψ: p ~ 0.1, g ~ 1e-3; w, g_i, h: p ~ 0.3, g ~ 0.1); ε (1e-3, 3e-3) is of the
    size of sqrt(v̂) for ψ and about a percent of it for the other groups, ten thousand bounds in either case."""
    id: str
    lr_psi: float
    wd_psi: float
    lr_w: float
    wd_w: float
    lr_g: float
    wd_g: float
    lr_h: float
    wd_h: float
    betas: Tuple[float, float]
    eps: float

    def of(self, group: str) -> Tuple[float, float]:
        """(lr, wd) of a group; the test phase's ω takes the g pair."""
        k = {"omega": "g"}.get(group, group)
        return getattr(self, "lr_" + k), getattr(self, "wd_" + k)

    def all_task(self) -> "HP":
        """The set the all-task paths run: lr_psi times ALL_TASK_LR (see there)."""
        return dataclasses.replace(self, lr_psi=self.lr_psi * ALL_TASK_LR)


# The all-task step updates the heads in order and head i's next actions are a GPI over all of them, so a measured
# step (earlier heads moved) and its recovery run (lr = 0: unmoved) see the same gradient only if those moves do not
# change an argmax.  With m0 / sqrt(v0) of order 1 every parameter moves by about lr; at the sets' lr_psi the T = 40
# case changes a next action, at 1/32 of it no case does on either minibatch (the float32 oracle's step:
# tests/test_adam_ref.py), so the all-task paths run at 1/64.  Both tests assert that the next actions agree.
ALL_TASK_LR = 2.0 ** -6
DEFAULTS = HP("defaults", 1e-3, 0.0, 1e-3, 0.0, 1e-3, 0.0, 1e-3, 0.0, (0.9, 0.999), 1e-8)
# β2 stays near enough to 1 that bc2 still moves from one step to the next at step 2000 (b2^2000 = 0.20 and 0.37):
# a stale or borrowed step count stays visible there, where bc1 already is 1 to float precision
HP_SETS = [
    DEFAULTS,
    HP("a", 7e-4, 2e-2, 1.3e-3, 0.6, 9e-4, 0.25, 1.7e-3, 0.4, (0.8, 0.9992), 1e-3),
    HP("b", 4e-4, 5e-3, 2.1e-3, 1.1, 1.5e-3, 0.35, 6e-4, 0.15, (0.95, 0.9995), 3e-3),
]
NON_DEFAULT = HP_SETS[1:]
K0S = (0, 3, 1997)   # loaded step counts: none (zero moments), a small one, one near 2000
RUNS = [(DEFAULTS, 3)] + [(hp, k0) for hp in NON_DEFAULT for k0 in K0S]   # the measured runs of every case


def f32(x: float) -> float:
    return float(np.float32(x))


def consts(lr: float, wd: float, betas, eps: float, step: int) -> Dict[str, float]:
    """adam_consts: the float32 constants of step number `step` (1-based), as doubles."""
    b1, b2 = betas
    bc1 = 1.0 - math.pow(b1, float(step))
    bc2 = 1.0 - math.pow(b2, float(step))
    return dict(omb1=f32(1.0 - b1), b2=f32(b2), omb2=f32(1.0 - b2), eps=f32(eps), wd=f32(wd),
                bc2s=f32(math.sqrt(bc2)), nss=f32(-(lr / bc1)) if bc1 != 0 else -math.inf)


def _d(x) -> torch.Tensor:
    return torch.as_tensor(x).detach().cpu().double().reshape(-1)


@dataclass
class Expect:
    p: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    bp: torch.Tensor
    bm: torch.Tensor
    bv: torch.Tensor

    def items(self):
        return (("p", self.p, self.bp), ("m", self.m, self.bm), ("v", self.v, self.bv))

    def sl(self, lo: int, hi: int) -> "Expect":
        return Expect(*(getattr(self, f.name)[lo:hi] for f in dataclasses.fields(self)))

    @staticmethod
    def cat(parts) -> "Expect":
        """Several groups (the heads of an all-task step, each with its own constants) as one."""
        return Expect(*(torch.cat([getattr(e, f.name) for e in parts]) for f in dataclasses.fields(Expect)))


def expect(p, g, m0, v0, c: Dict[str, float], floor: Optional[float] = None) -> Expect:
    """The recurrence in float64 on float32 inputs, and each output's bound (module docstring).
    floor: the clamp the caller puts on p' (the test phase's ω)."""
    p, g, m0, v0 = _d(p), _d(g), _d(m0), _d(v0)
    wd, omb1, b2, omb2 = c["wd"], c["omb1"], c["b2"], c["omb2"]
    G = g + wd * p
    M = m0 + omb1 * (G - m0)
    V = b2 * v0 + omb2 * G * G
    rt = V.sqrt()
    D = rt / c["bc2s"] + c["eps"]
    Q = c["nss"] * M / D
    P = p + Q
    eG = U * (g.abs() + 2 * (wd * p).abs()) if wd != 0 else torch.zeros_like(g)
    bm = omb1 * eG + U * (m0.abs() + 2 * omb1 * (G.abs() + m0.abs()))
    bv = 2 * omb2 * G.abs() * eG + U * (2 * b2 * v0 + 3 * omb2 * G * G)
    srt = torch.where(rt > 0, bv / (2 * rt).clamp_min(1e-300), torch.zeros_like(rt))
    eD = (srt + 2 * U * rt) / c["bc2s"] + U * D
    bp = U * P.abs() + abs(c["nss"]) * bm / D + Q.abs() * (eD / D + 2 * U)
    if floor is not None:
        P = P.clamp_min(floor)
    return Expect(P, M, V, bp * GUARD, bm * GUARD, bv * GUARD)


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
ROWS: List[Tuple[str, str, str, float, float]] = []   # (path, group, output, worst error / bound, |worst element|)


def ratios(got, want, bound, widen=None) -> torch.Tensor:
    """Per element |got - want| / bound; 0 / 0 is 0, anything else over a zero bound (or non-finite) is inf."""
    got, want, bound = _d(got), _d(want), _d(bound)
    if widen is not None:
        bound = bound + _d(widen)
    err = (got - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf).double())
    return torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))


def worst(got: Dict[str, torch.Tensor], e: Expect, widen: Optional[Expect] = None) -> Dict[str, Tuple[float, float]]:
    """Per output (p, m, v): (worst error in units of its bound, that element's expected magnitude)."""
    out = {}
    for k, want, bound in e.items():
        r = ratios(got[k], want, bound, None if widen is None else getattr(widen, k))
        assert r.numel() == want.numel(), f"{k}: {r.numel()} elements, expected {want.numel()}"
        j = int(r.argmax())
        out[k] = (float(r[j]), float(want[j].abs()))
    return out


def check(path: str, group: str, got: Dict[str, torch.Tensor], e: Expect, widen: Optional[Expect] = None):
    """Every element of p', m', v' within its bound; prints one row per output."""
    w = worst(got, e, widen)
    for k, (r, mag) in w.items():
        ROWS.append((path, group, k + "'", r, mag))
        print(f"| {path} | {group} | {k}' | {r:.3f} | {mag:.2e} |")
    for k, (r, mag) in w.items():
        assert r <= 1.0, f"{path} {group}: {k}' is {r:.3g} bounds off at an element of magnitude {mag:.3e}"


def spread(p, g_a, g_b, m0, v0, c, floor=None) -> Optional[Expect]:
    """The widening for a path whose two recovery runs differ: the spread of the two recovered gradients pushed
    through the float64 recurrence (None when they are bit-identical)."""
    if torch.equal(torch.as_tensor(g_a), torch.as_tensor(g_b)):
        return None
    a, b = expect(p, g_a, m0, v0, c, floor), expect(p, g_b, m0, v0, c, floor)
    z = torch.zeros_like(a.p)
    return Expect((a.p - b.p).abs(), (a.m - b.m).abs(), (a.v - b.v).abs(), z, z, z)


def assert_next_actions_agree(st, moved, spec, s1, what: str, gap: float = 1e-4):
    """The all-task step: head i's gradient depends on the heads before it only through its next actions (GPI over
    every head).  A recovery run (lr = 0) leaves those heads at st["online"], the measured run has moved them to
    `moved`; the recovered gradient is the measured run's if the float32 oracle picks the same next actions in both
    states with a top-2 gap of at least `gap` of max |q| (tests/test_gpu_gradients.py's margin)."""
    from tests import grad_ref as GR

    base = torch.as_tensor(st["online"]).float()
    moved = torch.as_tensor(moved).float()
    for i in range(base.shape[0]):
        mixed = base.clone()
        mixed[:i] = moved[:i]
        n0, g0 = GR.next_actions_of(base, st["w"][i], 0.0, spec, s1, i, True)
        n1, g1 = GR.next_actions_of(mixed, st["w"][i], 0.0, spec, s1, i, True)
        assert min(g0, g1) >= gap, f"{what} head {i}: next-action top-2 gap {min(g0, g1):.2e} of max |q|"
        assert torch.equal(n0, n1), f"{what} head {i}: the measured step's earlier heads change the next actions"


# ---------------------------------------------------------------------------------------------
# loaded state
# ---------------------------------------------------------------------------------------------
def loaded_moments(g, k0: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """float32 (m0, v0) for a group with gradient g: zero at k0 = 0, else m0 a normal draw at the scale (rms) of g
    and v0 a positive draw at the scale of its square, from a fixed generator."""
    g = torch.as_tensor(g).detach().cpu().float().reshape(-1)
    if k0 == 0:
        return torch.zeros_like(g), torch.zeros_like(g)
    gen = torch.Generator().manual_seed(7000 + seed)
    s = float(g.double().pow(2).mean().sqrt())
    assert s > 0
    m0 = torch.randn(g.numel(), generator=gen) * s
    v0 = (0.25 + 1.5 * torch.rand(g.numel(), generator=gen)) * (s * s)
    return m0.float(), v0.float()


# ---------------------------------------------------------------------------------------------
# the float32 oracle's step and its mutants (CPU)
# ---------------------------------------------------------------------------------------------
@dataclass
class Step:
    """What one group's step reads: float32 tensors and the group's knobs.  nb_step: a neighbouring head's step
    count; other: another group's (lr, wd)."""
    p: torch.Tensor
    g: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    step: int
    lr: float
    wd: float
    betas: Tuple[float, float]
    eps: float
    nb_step: int
    other: Tuple[float, float]

    def run(self, fn=None) -> Dict[str, torch.Tensor]:
        p, m, v = self.p.clone(), self.m.clone(), self.v.clone()
        if fn is None:
            R.adam_(p, self.g.clone(), m, v, self.step, self.lr, self.betas, self.eps, self.wd)
        else:
            fn(self, p, self.g.clone(), m, v)
        return dict(p=p, m=m, v=v)


def _tail(p, m, v, step, lr, betas, eps, inside=False, bc_step=None):
    b1, b2 = betas
    k = step if bc_step is None else bc_step
    bc1, bc2 = 1 - b1 ** k, 1 - b2 ** k
    if bc1 == 0 or bc2 == 0:   # bias corrections of step 0: the division by zero a stale step count runs into
        p.fill_(math.inf)
        return
    denom = (v / bc2).add_(eps).sqrt_() if inside else (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))


def _moments(g, m, v, betas, g_v=None):
    b1, b2 = betas
    m.lerp_(g, 1 - b1)
    gv = g if g_v is None else g_v
    v.mul_(b2).addcmul_(gv, gv, value=1 - b2)


def mut_no_decay(s, p, g, m, v):
    R.adam_(p, g, m, v, s.step, s.lr, s.betas, s.eps, 0.0)


def mut_decoupled(s, p, g, m, v):   # AdamW
    p.mul_(1 - s.lr * s.wd)
    R.adam_(p, g, m, v, s.step, s.lr, s.betas, s.eps, 0.0)


def mut_decay_after_moments(s, p, g, m, v):
    _moments(g, m, v, s.betas)
    bc1 = 1 - s.betas[0] ** s.step
    num = (m / bc1).add_(p, alpha=s.wd)
    denom = (v.sqrt() / ((1 - s.betas[1] ** s.step) ** 0.5)).add_(s.eps)
    p.addcdiv_(num, denom, value=-s.lr)


def mut_betas_swapped(s, p, g, m, v):
    R.adam_(p, g, m, v, s.step, s.lr, (s.betas[1], s.betas[0]), s.eps, s.wd)


def mut_stale_step(s, p, g, m, v):
    g = g.add(p, alpha=s.wd)
    _moments(g, m, v, s.betas)
    _tail(p, m, v, s.step, s.lr, s.betas, s.eps, bc_step=s.step - 1)


def mut_neighbour_step(s, p, g, m, v):
    g = g.add(p, alpha=s.wd)
    _moments(g, m, v, s.betas)
    _tail(p, m, v, s.step, s.lr, s.betas, s.eps, bc_step=s.nb_step)


def mut_eps_inside(s, p, g, m, v):
    g = g.add(p, alpha=s.wd)
    _moments(g, m, v, s.betas)
    _tail(p, m, v, s.step, s.lr, s.betas, s.eps, inside=True)


def mut_v_before_decay(s, p, g, m, v):
    _moments(g.add(p, alpha=s.wd), m, v, s.betas, g_v=g)
    _tail(p, m, v, s.step, s.lr, s.betas, s.eps)


def mut_other_group(s, p, g, m, v):   # ψ with (lr_w, wd_w), w with (lr_psi, wd_psi)
    R.adam_(p, g, m, v, s.step, s.other[0], s.betas, s.eps, s.other[1])


MUTANTS = dict(no_decay=mut_no_decay, decoupled=mut_decoupled, decay_after_moments=mut_decay_after_moments,
               betas_swapped=mut_betas_swapped, stale_step=mut_stale_step, neighbour_step=mut_neighbour_step,
               eps_inside=mut_eps_inside, v_before_decay=mut_v_before_decay, other_group=mut_other_group)
OTHER = dict(psi="w", w="psi", g="h", h="g", omega="w")   # whose (lr, wd) the other_group mutant borrows


def step_of(group: str, p, g, hp: HP, k0: int, seed: int, nb: int = 1) -> Step:
    """The measured run of one group on the CPU: float32 inputs, moments loaded at step k0."""
    p, g = torch.as_tensor(p).detach().float().reshape(-1).clone(), torch.as_tensor(g).detach().float().reshape(-1).clone()
    m0, v0 = loaded_moments(g, k0, seed)
    lr, wd = hp.of(group)
    return Step(p, g, m0, v0, k0 + 1, lr, wd, hp.betas, hp.eps, k0 + 1 + nb, hp.of(OTHER[group]))


def expect_of(s: Step, floor=None) -> Expect:
    return expect(s.p, s.g, s.m, s.v, consts(s.lr, s.wd, s.betas, s.eps, s.step), floor)
