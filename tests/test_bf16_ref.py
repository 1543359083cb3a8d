"""The bf16 emulation and its probes (tests/bf16_ref.py) on the CPU: the rounding is pinned, the emulated Linear's
autograd is checked against a hand-written backward, the carriers are exact, and every mutant of the emulation --
the ways a bf16 kernel goes subtly wrong -- leaves the bounds the GPU tests (tests/test_gpu_bf16_values.py) assert
at the same shapes, with the float32 emulation standing in for the GPU."""
import pytest
import torch

from tests import bf16_ref as B
from tests import grad_ref as G

F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------
# q
# ---------------------------------------------------------------------------------------------
def _edge_values():
    one = torch.tensor([1.0, 1.5, 0.1, 3.0, 255.0, 2.0 ** -100, 2.0 ** 100], dtype=F32)
    ulp = one.abs() * 2.0 ** -7   # at most one bf16 ulp of each value
    steps = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.5, 127.5, 128.5]).view(-1, 1) * 2.0 ** -1
    x = (one + steps * ulp).reshape(-1)   # exact in float32: ties to an even and to an odd neighbour included
    top = torch.tensor([0x7F7F0000, 0x7F7E8000, 0x00800000, 0x00808000, 0x3F80FFFF, 0x3F808000, 0x3F818000,
                        0x3F808001, 0x3F807FFF], dtype=torch.int32).view(F32)   # largest bf16, smallest normal, ties
    x = torch.cat([x, top, torch.zeros(1)])
    return torch.cat([x, -x])


def test_q_is_rne_to_bf16():
    gen = torch.Generator().manual_seed(0)
    x = torch.cat([_edge_values(), torch.randn(100000, generator=gen),
                   torch.randn(20000, generator=gen) * 1e-20, torch.randn(20000, generator=gen) * 1e20])
    want = x.to(torch.bfloat16).to(F32)
    assert torch.equal(B.q(x), want)
    assert B.q(x).dtype == F32
    q64 = B.q(x.double())
    assert q64.dtype == F64 and torch.equal(q64, want.double())
    assert torch.equal(B.q(B.q(x)), B.q(x))
    t = B.trunc(x)
    assert bool((t.abs() <= x.abs()).all()) and torch.equal(t.view(torch.int32) & 0xFFFF, torch.zeros_like(t, dtype=torch.int32))
    assert bool((B.trunc(x.double()) == t.double()).all())


def test_q_has_no_double_rounding():
    """1 + 2^-8 + 2^-30 is above the midpoint of 1 and 1 + 2^-7: it rounds up.  Through float32 it first becomes
    the midpoint itself and then ties to the even 1."""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, -(1.0 + 2.0 ** -8 + 2.0 ** -30)], dtype=F64)
    assert B.q(x).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]
    assert x.float().to(torch.bfloat16).double().tolist() == [1.0, -1.0]


# ---------------------------------------------------------------------------------------------
# the emulated Linear
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fwd_bf16,dx_bf16", [(True, True), (False, True), (True, False), (False, False)])
def test_linear_autograd_matches_hand_written_backward(fwd_bf16, dx_bf16):
    gen = torch.Generator().manual_seed(1)
    x, W, b = (torch.randn(*s, generator=gen, dtype=F64).requires_grad_(True) for s in ((5, 24), (9, 24), (9,)))
    dz = torch.randn(5, 9, generator=gen, dtype=F64)
    z = B.linear(x, W, b, fwd_bf16, dx_bf16)
    z.backward(dz)
    xd, Wd = x.detach(), W.detach()
    assert torch.equal(z.detach(), (B.q(xd) @ B.q(Wd).T if fwd_bf16 else xd @ Wd.T) + b.detach())
    assert torch.equal(x.grad, B.q(dz) @ B.q(Wd) if dx_bf16 else dz @ Wd)
    assert torch.equal(W.grad, dz.T @ xd) and torch.equal(b.grad, dz.sum(0))
    if not fwd_bf16 and not dx_bf16:   # and the plain one is F.linear
        x2, W2, b2 = (v.detach().clone().requires_grad_(True) for v in (x, W, b))
        torch.nn.functional.linear(x2, W2, b2).backward(dz)
        for a, c in ((x, x2), (W, W2), (b, b2)):
            torch.testing.assert_close(a.grad, c.grad, rtol=1e-13, atol=1e-13)


def test_grad_ref_mlp_takes_the_emulated_linear():
    g = B.Geo(17, 32, 3, 4, 1)
    gen = torch.Generator().manual_seed(2)
    flat, X = torch.randn(g.P, generator=gen, dtype=F64), torch.randn(6, 17, generator=gen, dtype=F64)
    acts = (None,) + g.acts + (None,)
    plain = G.mlp(flat, g.dims, acts, X)
    assert torch.equal(plain, G.mlp(flat, g.dims, acts, X, linear=B.layerwise([False] * 3, [False] * 3)))
    fm = B.fwd_map(g, 6)
    assert fm == [False, True, True]
    emu = G.mlp(flat, g.dims, acts, X, linear=B.layerwise(fm, B.dx_map(g, 2)))
    assert not torch.equal(plain, emu) and float((plain - emu).abs().max()) < 0.1 * float(plain.abs().max())


# ---------------------------------------------------------------------------------------------
# the dispatch map
# ---------------------------------------------------------------------------------------------
def test_map_examples():
    g = B.Geo(17, 256, 7, 8)
    assert B.fused01(g) and B.fwd_map(g, 32) == [False, True, True, True]
    assert B.fwd_map(g, 32, bf16=False) == [False] * 4
    assert B.fwd_map(B.Geo(17, 40, 7, 8), 32) == [False] * 4                 # K % 32 != 0: fp32 forward ...
    assert B.dx_map(B.Geo(17, 40, 7, 8), 3) == [False, True, True, False]   # ... bf16 dX, fused TD launch fp32
    assert B.dx_map(B.Geo(11, 64, 27, 50), 3) == [False, True, True, True]  # A·d > 128: a plain last dX tile
    assert B.fwd_map(B.Geo(17, 64, 64, 8), 4) == [False, True, True, False]  # the GEMV of N = 512 at M <= 4
    assert B.fwd_map(B.Geo(17, 64, 64, 8), 5) == [False, True, True, True]
    assert not B.fused01(B.Geo(32, 48, 4, 8)) and not B.fused01(B.Geo(96, 64, 4, 8))
    assert B.fwd_map(B.Geo(32, 48, 4, 8), 17) == [False] * 4 and not B.fwd_map(B.Geo(96, 64, 4, 8), 17)[0]
    assert B.fwd_map(B.Geo(32, 48, 4, 8), 17, aligned=False) == [False] * 4
    # two column tiles per workgroup from 384 tiles on: T = 24 heads of 16 column tiles, and not one head fewer
    assert B.tp2_tiles(256, 17, 24) == (384, True) and not B.tp2_tiles(256, 17, 23)[1]
    assert B.tp2_tiles(264, 17, 24) == (408, True)   # 17 column tiles: the last workgroup has one


def test_probe_ids_are_unique_and_tp2_cases_reach_it():
    ids = [p.id for p in B.FWD_PROBES + B.UPD_PROBES] + [p.id for p in B.BWD_PROBES]
    assert len(set(ids)) == len(ids)
    for p in B.FWD_PROBES:
        N = p.geo.dims[p.under][0]
        assert B.tp2_tiles(N, p.M, p.T)[1] == p.id.startswith("tp2"), p.id


# ---------------------------------------------------------------------------------------------
# forward probes: carriers exact, the float32 emulation inside the check, the mutants outside
# ---------------------------------------------------------------------------------------------
FWD = {p.id: p for p in B.FWD_PROBES + B.UPD_PROBES}
_cache = {}


def problem(p):
    if p.id not in _cache:
        heads, S = B.carrier_heads(p), B.probe_inputs(p)
        _cache[p.id] = (heads, S, B.run_probe(p, heads, S, F64))
    return _cache[p.id]


@pytest.mark.parametrize("pid", list(FWD))
def test_carriers_are_exact_and_fp32_emulation_passes(pid):
    p = FWD[pid]
    heads, S, r64 = problem(p)
    r32 = B.run_probe(p, heads, S, F32)
    # what the carriers deliver to the layer under test: bit-identical in both emulations
    assert torch.equal(r32.x.double(), r64.x)
    if p.under < p.geo.NL - 1:   # and what the carriers above make of the float32 run's own z: exactly post(z)
        unit, scale = B._select(p, heads)
        z = r32.z.gather(2, unit.unsqueeze(0).expand(p.M, -1, -1))
        want = (B.q(torch.relu(z)) if r64.rounded_above else torch.relu(z)) * scale.float()
        assert torch.equal(r32.psi.reshape(want.shape), want)
        assert B.units_seen(p, heads) == min(p.geo.dims[p.under][0], p.T * p.geo.A * p.geo.d)
    ratio, n, bad = B.check_probe(p, heads, r32.psi, r64)
    assert bad == 0, (pid, ratio, bad, n)
    # the inputs are not bf16-representable: the RNE of X and of the copy is under test
    (N, K), (w0, w1) = p.geo.dims[p.under], p.geo.offsets()[p.under]
    assert float((B.q(heads[:, w0:w1]) != heads[:, w0:w1]).float().mean()) > 0.9
    assert float((B.q(S) != S).float().mean()) > 0.9


def stale(heads, p):
    """The layer under test from before an Adam step of lr = 1e-3 (a first step moves every weight by ±lr)."""
    gen = torch.Generator().manual_seed(5)
    w0, w1 = p.geo.offsets()[p.under]
    out = heads.clone()
    out[:, w0:w1] += 1e-3 * (torch.randint(0, 2, (heads.shape[0], w1 - w0), generator=gen) * 2 - 1)
    return out


FWD_MUTANTS = {
    "x_truncated": dict(qx=B.trunc),
    "w_truncated": dict(qw=B.trunc),
    "w_unrounded": dict(qw=B.ident),
    "x_unrounded": dict(qx=B.ident),
    "k_group_dropped": dict(kgroup=1),
    "k_group_duplicated": dict(kgroup=-1),
    "w_stale": None,
}


@pytest.mark.parametrize("mutant", list(FWD_MUTANTS))
@pytest.mark.parametrize("pid", list(FWD))
def test_forward_mutants_leave_the_bounds(pid, mutant):
    p = FWD[pid]
    heads, S, r64 = problem(p)
    fmap = B.fwd_map(p.geo, p.M, p.aligned)
    if mutant == "w_stale":
        got = B.run_probe(p, stale(heads, p), S, F32).psi
    elif fmap[p.under] or "k_group" in mutant:
        got = B.run_probe(p, heads, S, F32, ops=B.Ops(**FWD_MUTANTS[mutant])).psi
    else:   # an fp32 product by the map: there the operand mutants are one, the product run in bf16
        got = B.run_probe(p, heads, S, F32, fmap=[f or l == p.under for l, f in enumerate(fmap)]).psi
    ratio, n, bad = B.check_probe(p, heads, got, r64)
    print(f"{pid} {mutant}: {bad}/{n} outside, worst error / bound {ratio:.3g}")
    # (x_unrounded is required of the last-layer probes; the hidden-layer probes, which observe at bf16 resolution,
    # reject it as well: about half of their outputs fall outside)
    assert bad > 0, (pid, mutant, ratio)


# ---------------------------------------------------------------------------------------------
# backward probes: the read-out is exact, the mutants leave the bound
# ---------------------------------------------------------------------------------------------
BWD = {p.id: p for p in B.BWD_PROBES}


def emulated_moments(p, bf16, ops=B.SPEC, dtype=F32):
    """The gradient of one head's TD-shaped loss through the emulated network: what the recovery step leaves in the
    first moments.  -> (flat gradient, W_1 master)."""
    g = p.geo
    heads, _, (S, a, r, phi, S1, gamma), i, j = B.bwd_problem(p)
    flat = heads[0].to(dtype).clone().requires_grad_(True)
    fm, dm = B.fwd_map(g, p.B, bf16=bf16), B.dx_map(g, p.T, bf16=bf16)
    out = G.mlp(flat, g.dims, (None,) + g.acts + (None,), S.to(dtype), linear=B.layerwise(fm, dm, ops))
    tgt = torch.zeros_like(out)
    tgt[:, :g.d] = phi.to(dtype)
    ((out - tgt.detach()) ** 2).mean().backward()
    w0, w1 = g.offsets()[1]
    return flat.grad.detach(), heads[0, w0:w1].view(g.H, g.H)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("pid", list(BWD))
def test_backward_readout_is_exact_and_emulation_passes(pid, bf16):
    p = BWD[pid]
    grad, W1 = emulated_moments(p, bf16)
    _, _, _, i, j = B.bwd_problem(p)
    dz1, dz0, db1 = B.bwd_readout(p, grad, i, j)
    assert bool(dz1.any()) and bool(dz0.any())
    ref, bound = B.dx_reference(p, W1, dz1, bf16)
    ratio, n, bad = B.dx_verdict(dz0, ref, bound)
    assert bad == 0 and n == p.B * p.geo.H, (pid, ratio, bad)
    assert B.db_verdict(dz1, db1) <= 1.0
    # every other column of dW_0 and dW_1 is exactly zero: the rows are basis vectors
    g = p.geo
    (a0, a1), (b0, b1) = g.offsets()[0], g.offsets()[1]
    mask0, mask1 = torch.ones(g.n_s, dtype=torch.bool), torch.ones(g.H, dtype=torch.bool)
    mask0[i], mask1[j] = False, False
    assert not bool(grad[a0:a1].view(g.H, g.n_s)[:, mask0].any())
    assert not bool(grad[b0:b1].view(g.H, g.H)[:, mask1].any())
    if bf16:   # the other precision's emulation is outside the bound: the read-out is exact, not merely loose
        ref_o, bound_o = B.dx_reference(p, W1, dz1, False)
        assert B.dx_verdict(dz0, ref_o, bound_o)[2] > 0


BWD_MUTANTS = {
    "dz_unrounded": dict(qdz=B.ident),
    "dz_truncated": dict(qdz=B.trunc),
    "w_truncated": dict(qwdx=B.trunc),
    "w_unrounded": dict(qwdx=B.ident),
    "k_group_dropped": dict(kgroup=1),
    "k_group_duplicated": dict(kgroup=-1),
    "dx_as_forward": dict(dx_as_fwd=True),
}


@pytest.mark.parametrize("mutant", list(BWD_MUTANTS) + ["w_stale"])
@pytest.mark.parametrize("pid", list(BWD))
def test_backward_mutants_leave_the_bound(pid, mutant):
    p = BWD[pid]
    _, _, _, i, j = B.bwd_problem(p)
    if mutant == "w_stale":   # the reference given the weights one lr = 1e-3 step on: the copy the GPU read is stale
        grad, W1 = emulated_moments(p, True)
        gen = torch.Generator().manual_seed(6)
        W1 = W1 + 1e-3 * (torch.randint(0, 2, W1.shape, generator=gen) * 2 - 1)
    else:
        grad, W1 = emulated_moments(p, True, B.Ops(**BWD_MUTANTS[mutant]))
    dz1, dz0, _ = B.bwd_readout(p, grad, i, j)
    ref, bound = B.dx_reference(p, W1, dz1, True)
    ratio, n, bad = B.dx_verdict(dz0, ref, bound)
    print(f"{pid} {mutant}: {bad}/{n} outside, worst error / bound {ratio:.3g}")
    if mutant == "dx_as_forward" and B.fwd_map(p.geo, p.B)[1]:
        assert bad == 0   # the forward is bf16 too: not a mutant at this shape
        return
    assert bad > 0, (pid, mutant, ratio)


# ---------------------------------------------------------------------------------------------
# composition cases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.COMP_CASES, ids=lambda c: c.id)
def test_composition_seeds_keep_their_conditions(c):
    """The committed seeds: no X or dZ operand within 2^-19 of a bf16 midpoint in either emulation (a rounding flip
    would move the gradient by more than the comparison allows), and the kinks of tests/grad_ref.py stay clear."""
    (pc, st, b), g64, r32, info, dist = B.comp_oracles(c)
    info.check(c.id)
    assert dist > B.MID
    assert B.dx_map(c.geo, c.T)[-1] == (c.id == "plain_last_dx")
    bound, e32, scale = G.grad_bound(g64["psi"], r32["psi"])
    # and the comparison tells the precisions apart: the fp32 network's gradient is outside the bf16 one's bound
    _, f64, _, _, _ = B.comp_oracles(c, bf16=False)
    assert float((f64["psi"] - g64["psi"]).abs().max()) > 10 * bound
