"""bf16 operand mode by value: the emulation, the dispatch map, the probes and their bounds, for
tests/test_bf16_ref.py (CPU) and tests/test_gpu_bf16_values.py.  No GPU import.

The mode: a bf16 product is sum_k q(x_k) q(w_k) accumulated in fp32, q = round to nearest even to
bf16; x is rounded in registers, w is read from a copy that must be q(master) at all times; the bias add, the
activations, dW and Adam stay fp32.  Which products are bf16 is decided on the host, and `fwd_map` / `dx_map`
restate that decision from DESIGN.md; a shape at which the library decides otherwise fails the GPU tests.

A whole-network comparison cannot tell a wrong operand from a rounding flip (a hidden activation within an fp32
error of a bf16 midpoint rounds the other way on the GPU and moves ψ by up to 3e-3 of its scale, as much as a
truncated operand does).  So the probes isolate ONE product whose operands are known exactly:

  * forward: carrier heads.  Every layer but the one under test has rows with a single power-of-two weight and no
    bias, ReLU carriers only ever see inputs >= 0: a carrier copies exactly in fp32 and yields exactly q(x) in bf16.
    The layer under test has ordinary random fp32 weights.  Under test last: ψ is the product, every element within
    `bound` of the float64 emulation.  Under test hidden: the carriers above deliver q(relu(z)) of selected units
    (every head other units), each of which must be a bf16 value in [q(relu(z64 - bound)), q(relu(z64 + bound))]:
    one of the two ends, but for units so close to zero that bf16 is finer than the fp32 sum's error;
  * backward: basis rows through a carrier layer 0, so that with the recovery recipe of tests/test_gpu_adam.py
    (lr = 0, β1 = 0, zero moments) dW_1[n, j(m)] = dZ_1[m, n] and dW_0[j, i(m)] = dZ_0[m, j] bit for bit: the layer-1
    dX is checked from the GPU's own dZ_1 bits.

bound = 2 (K+1) 2^-24 (sum_k |x_k w_k| + |b|) over the operands as multiplied: twice the textbook bound of a
length-(K+1) fp32 sum in any order (the MFMA's internal order and rounding are not documented).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24

# the host's constants the map depends on (csrc/sfx_kernels.h)
L0_KMAX, L0_NMAX = 64, 256      # layer 0 computed inside the layer-1 tiles (fp32)
GEMV_M, GEMV_N = 4, 512         # few rows of a wide layer: the fp32 GEMV
NCU = 256
TDG_O, TDG_A = 128, 128         # the fused TD launch (fp32 last-layer dX): A·d <= 128, A <= 128, d % 4 == 0


# ---------------------------------------------------------------------------------------------
# rounding
# ---------------------------------------------------------------------------------------------
def _drop(x: torch.Tensor, rne: bool) -> torch.Tensor:
    """x with its significand cut to bf16's 8 bits, by RNE or truncation, in x's dtype (one rounding of the
    value x holds; finite normal bf16 range only)."""
    assert x.dtype in (F32, F64)
    bits, n = (x.contiguous().view(torch.int32), 16) if x.dtype == F32 else (x.contiguous().view(torch.int64), 45)
    if rne:
        bits = bits + ((1 << (n - 1)) - 1) + ((bits >> n) & 1)   # sign-magnitude: the carry rounds |x|
    bits = (bits >> n) << n
    return bits.view(x.dtype).reshape(x.shape)


def q(x: torch.Tensor) -> torch.Tensor:
    """Round to nearest even to bf16, without double rounding, in x's dtype (float32 or float64)."""
    return _drop(x, True)


def trunc(x: torch.Tensor) -> torch.Tensor:
    return _drop(x, False)


def ident(x: torch.Tensor) -> torch.Tensor:
    return x


# ---------------------------------------------------------------------------------------------
# one product
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Ops:
    """How the operands of a bf16 product are prepared.  The defaults are the specification; anything else is a
    mutant (tests/test_bf16_ref.py) that the probes' checks must reject."""
    qx: Callable = q          # forward X
    qw: Callable = q          # forward W (the copy)
    qdz: Callable = q         # dX: dZ
    qwdx: Callable = q        # dX: W (the copy)
    kgroup: int = 0           # +1: one 8-wide k group dropped, -1: one duplicated (the second of the product)
    dx_as_fwd: bool = False   # the dX takes the forward's precision (fp32 where the forward is)


SPEC = Ops()


def _kg(x, w, ops):
    if ops.kgroup and x.shape[-1] >= 16:
        g = slice(8, 16)
        x = x.clone()
        x[..., g] = 0 if ops.kgroup > 0 else 2 * x[..., g]
    return x, w


def product(x, W, b, bf16: bool, ops: Ops = SPEC):
    """(z [M, N], bound [M, N]) of x [M, K] @ W [N, K]^T + b in the dtype of x (float64: the reference)."""
    xo, wo = (ops.qx(x), ops.qw(W)) if bf16 else (x, W)
    xo, wo = _kg(xo, wo, ops)
    z = xo @ wo.T
    mag = xo.abs() @ wo.abs().T
    if b is not None:
        z, mag = z + b, mag + b.abs()
    return z, 2.0 * (x.shape[-1] + 1) * U * mag


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, fwd_bf16, dx_bf16, ops):
        ctx.save_for_backward(x, W)
        ctx.dx_bf16, ctx.ops = dx_bf16, ops
        return product(x, W, b, fwd_bf16, ops)[0]

    @staticmethod
    def backward(ctx, dz):
        x, W = ctx.saved_tensors
        ops = ctx.ops
        dx = (ops.qdz(dz) @ ops.qwdx(W)) if ctx.dx_bf16 else dz @ W
        return dx, dz.T @ x, dz.sum(0), None, None, None   # dW, db from the unrounded values


def linear(x, W, b, fwd_bf16: bool, dx_bf16: bool, ops: Ops = SPEC):
    """The emulated Linear: forward q(x) @ q(W)^T + b or plain, dX = q(dZ) @ q(W) or plain, dW and db plain."""
    return _Linear.apply(x, W, b, fwd_bf16, dx_bf16, ops)


def layerwise(fwd: List[bool], dx: List[bool], ops: Ops = SPEC):
    """A `linear=` argument of tests/grad_ref.mlp: call i of a network's forward is layer i of the maps."""
    it = iter(range(len(fwd)))

    def f(x, W, b):
        l = next(it)
        return linear(x, W, b, fwd[l], fwd[l] if ops.dx_as_fwd else dx[l], ops)

    return f


# ---------------------------------------------------------------------------------------------
# the dispatch map
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Geo:
    n_s: int
    H: int
    A: int
    d: int
    n_hidden: int = 2

    @property
    def acts(self):
        return ("relu",) * self.n_hidden

    @property
    def NL(self):
        return self.n_hidden + 2

    @property
    def dims(self):   # (N, K) per layer
        return [(self.H, self.n_s)] + [(self.H, self.H)] * self.n_hidden + [(self.A * self.d, self.H)]

    @property
    def P(self):
        return sum(n * k + n for n, k in self.dims)

    def offsets(self):
        out, off = [], 0
        for n, k in self.dims:
            out.append((off, off + n * k))
            off += n * k + n
        return out


def fused01(g: Geo) -> bool:
    """Layers 0 and 1 in one launch, layer 0 in-tile (fp32)."""
    return g.NL >= 3 and g.n_s <= L0_KMAX and g.H <= L0_NMAX and g.H % 32 == 0


def fwd_map(g: Geo, M: int, aligned: bool = True, bf16: bool = True) -> List[bool]:
    """Per layer: does a forward of M rows from layer 0 take bf16 operands?  A layer is bf16 iff it runs on the
    vector path (K % 32 == 0, 16-byte aligned input) and is neither the few-row GEMV nor layer 0."""
    out = []
    for l, (N, K) in enumerate(g.dims):
        if l == 0:
            out.append(False)   # fp32 wherever it runs: in-tile, inside the dW tiles, as a launch of its own
        else:
            gemv = not (l == 1 and fused01(g)) and M <= GEMV_M and N >= GEMV_N and K % 16 == 0
            out.append(bf16 and not gemv and K % 32 == 0)
    return out


def tdg_fused(g: Geo, T: int) -> bool:
    """The fused TD launch computes the last layer's dX in fp32."""
    if g.d % 4 or g.A * g.d > TDG_O or g.A > TDG_A:
        return False
    return (g.d <= 8 and 32 * T * g.A <= 2048) or (g.d <= 16 and 32 * T * g.A <= 1024)


def dx_map(g: Geo, T: int, bf16: bool = True) -> List[bool]:
    """Per layer l: is dZ_{l-1} = dZ_l W_l a bf16 product?  Every plain dX tile is, whatever K; the fused TD
    launch's last-layer dX is not; layer 0 has no dX."""
    return [bf16 and l > 0 and not (l == g.NL - 1 and tdg_fused(g, T)) for l in range(g.NL)]


def tp2_tiles(N: int, M: int, ninst: int) -> Tuple[int, bool]:
    """(16x32 tiles of one forward launch over ninst heads, two column tiles per workgroup?) by the host's rule:
    2 tiles >= 3 ncu, tiles <= 4 ncu, more than one column tile."""
    ntN = -(-N // 16)
    tiles = ntN * -(-M // 32) * ninst
    return tiles, ntN > 1 and 2 * tiles >= 3 * NCU and tiles <= 4 * NCU


# ---------------------------------------------------------------------------------------------
# forward probes: carrier heads
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Probe:
    id: str
    geo: Geo
    T: int
    M: int
    under: int                 # the layer under test (NL - 1: the last)
    reaches: str = ""          # the instantiation the case is there for (profiles/bf16_error.md)
    seed: int = 0
    aligned: bool = True


def _carrier(N, K, shift):
    """[N, K]: row j has the single weight 2^-(j // K mod 4) at column (j + shift) mod K."""
    W = torch.zeros(N, K)
    j = torch.arange(N)
    W[j, (j + shift) % K] = 2.0 ** -((j // K) % 4).float()
    return W


def carrier_heads(p: Probe) -> torch.Tensor:
    """[T, P] float32 in torch packing: random reference-initialised weights in layer `under`, carriers elsewhere.
    Head t's last layer is rotated by t·A·d (the hidden carriers by 5 in every head), so that with a hidden layer under test the heads' outputs select
    different units (all H of them once T·A·d >= H)."""
    from sfx.init import reference_heads

    g = p.geo
    heads, _ = reference_heads(p.T, g.n_s, g.H, g.A, g.d, g.acts, seed=500 + p.seed)
    heads = heads.clone()
    for t in range(p.T):
        for l, ((N, K), (w0, w1)) in enumerate(zip(g.dims, g.offsets())):
            if l == p.under:
                continue
            shift = t * g.A * g.d if l == g.NL - 1 else (5 if l > 0 else 0)
            heads[t, w0:w1] = _carrier(N, K, shift).reshape(-1)
            heads[t, w1:w1 + N] = 0
    return heads


def probe_inputs(p: Probe) -> torch.Tensor:
    """S [M, n_s] > 0, random float32 (not bf16-representable)."""
    gen = torch.Generator().manual_seed(7000 + p.seed)
    return torch.rand(p.M, p.geo.n_s, generator=gen) * 1.5 + 0.05


@dataclass
class Trace:
    psi: torch.Tensor                  # [M, T, A, d]
    z: torch.Tensor                    # [M, T, N_under]: the product under test (before its activation)
    bound: torch.Tensor
    rounded_above: bool                # a bf16 layer reads the layer under test's output
    x: torch.Tensor = None             # [M, T, K_under]: what the carriers below deliver to the layer under test


def run_probe(p: Probe, heads: torch.Tensor, S: torch.Tensor, dtype=F64, bf16: bool = True, ops: Ops = SPEC,
              fmap: Optional[List[bool]] = None) -> Trace:
    """The emulation of one forward through every head in `dtype`.  ops apply to every bf16 product, as a wrong
    kernel would: X's rounding shows at the first bf16 layer (a carrier, unless the layer under test is it)."""
    g = p.geo
    fmap = fwd_map(g, p.M, p.aligned, bf16) if fmap is None else fmap
    psis, zs, bs, xs = [], [], [], []
    for t in range(heads.shape[0]):
        y = S.to(dtype)
        for l, ((N, K), (w0, w1)) in enumerate(zip(g.dims, g.offsets())):
            W, b = heads[t, w0:w1].view(N, K).to(dtype), heads[t, w1:w1 + N].to(dtype)
            z, bound = product(y, W, b, fmap[l], ops)
            if l == p.under:
                xs.append(y)
                zs.append(z)
                bs.append(bound)
            y = torch.relu(z) if 0 < l < g.NL - 1 else z
        psis.append(y)
    return Trace(torch.stack(psis, 1).view(p.M, -1, g.A, g.d), torch.stack(zs, 1), torch.stack(bs, 1),
                 p.under < g.NL - 1 and fmap[p.under + 1], torch.stack(xs, 1))


def _select(p: Probe, heads: torch.Tensor):
    """Hidden under test: which unit of layer `under` each ψ output of each head carries, and the power of two
    it is scaled by on the way up -- read off the carriers themselves."""
    g = p.geo
    units, scales = [], []
    for t in range(heads.shape[0]):
        idx, sc = None, None
        for l in range(g.NL - 1, p.under, -1):
            (N, K), (w0, w1) = g.dims[l], g.offsets()[l]
            W = heads[t, w0:w1].view(N, K)
            col, val = W.abs().argmax(1), W.abs().amax(1)
            idx, sc = (col, val) if idx is None else (col[idx], sc * val[idx])
        units.append(idx)
        scales.append(sc)
    return torch.stack(units), torch.stack(scales)


def check_probe(p: Probe, heads: torch.Tensor, got: torch.Tensor, ref: Trace) -> Tuple[float, int, int]:
    """got: ψ [M, T, A, d] of the library (or of a mutant).  -> (worst error / bound, elements compared,
    elements outside the check).  Last layer under test: |got - z64| <= bound.  Hidden layer under test: each
    output lies in [post(z64 - bound), post(z64 + bound)] of the unit it carries, post = the carriers' scale times
    relu, rounded to bf16 (and then the output is a bf16 value too) when a bf16 layer reads the unit."""
    g = p.geo
    got = got.detach().cpu().double().reshape(p.M, heads.shape[0], -1)
    if p.under == g.NL - 1:
        err = (got - ref.z).abs()
        ratio = torch.where(ref.bound > 0, err / ref.bound.clamp(min=1e-300), torch.where(err > 0, 1e30, 0.0))
        return float(ratio.max()), got.numel(), int((err > ref.bound).sum())
    unit, scale = _select(p, heads)
    ix = unit.unsqueeze(0).expand(p.M, -1, -1)
    z, b = ref.z.gather(2, ix), ref.bound.gather(2, ix)
    post = (lambda v: q(torch.relu(v)) * scale) if ref.rounded_above else (lambda v: torch.relu(v) * scale)
    lo, hi = post(z - b), post(z + b)
    # post is monotone: a z within the bound lands in [lo, hi].  (Interval plus representability IS membership in
    # {lo, hi} whenever no third bf16 value lies between the two.)  Rounded, that is lo or hi themselves wherever the
    # interval holds no third bf16 value (all but the units with |z| below ~2^8 bounds, where bf16 is finer than
    # the fp32 sum's error): there the output must be one of the bf16 values in between
    bad = (got < lo) | (got > hi)
    if ref.rounded_above:
        bad |= q(got) != got
    ratio = ((got - post(z)).abs() / (b * scale).clamp(min=1e-300)).max()
    return float(ratio), got.numel(), int(bad.sum())


def units_seen(p: Probe, heads: torch.Tensor) -> int:
    return int(_select(p, heads)[0].unique().numel())


G2 = lambda n_s, H, A=7, d=8, nh=2: Geo(n_s, H, A, d, nh)
LAST = lambda g: g.NL - 1

FWD_PROBES: List[Probe] = (
    # plain vector tile, one column tile per workgroup: half-valid row blocks, a second row tile
    [Probe(f"last_H{H}_M{M}", G2(17, H), 2, M, 3, "k_fwd<true,false,true,1> last layer")
     for H in (32, 64) for M in (1, 7, 16, 17, 32, 33)]
    # K edges: one wave's chunk, all eight waves once, a second pass of one wave only, two passes
    + [Probe(f"last_K{H}", G2(17, H), 2, 9, 3, f"k_fwd<true,false,true,1> K = {H}") for H in (256, 288, 512)]
    # N edges: a half-full last column tile, a single tile, N no multiple of 8
    + [Probe("last_N56", G2(17, 64, 7, 8), 2, 9, 3, "N = 56: last 16-column tile half full"),
       Probe("last_N16", G2(17, 64, 2, 8), 2, 9, 3, "N = 16: one column tile"),
       Probe("last_N51", G2(17, 64, 3, 17), 2, 9, 3, "N = 51: not a multiple of 8")]
    # hidden layers: layer 1 inside the fused layer-0+1 launch (n_s = 4, 17, 64), layer 2 as a plain tile
    + [Probe(f"l1_fused_ns{n}", G2(n, 64, 4, 8), 2, 17, 1, "k_fwd<true,true,true,1> layer 1") for n in (4, 17, 64)]
    + [Probe("l1_plain_ns96", G2(96, 64, 4, 8), 2, 17, 1, "k_fwd<true,false,true,1> layer 1, X from an fp32 layer 0"),
       Probe("last_ns96_one_hidden", G2(96, 64, 4, 8, 1), 2, 17, 2, "k_fwd<true,false,true,1> last layer, K0 > 64"),
       Probe("l2_H64", G2(17, 64, 4, 8), 2, 17, 2, "k_fwd<true,false,true,1> hidden layer"),
       Probe("l2_H288", G2(17, 288, 9, 8), 4, 9, 2, "k_fwd<true,false,true,1> hidden, K = 288"),
       Probe("l1_one_hidden", G2(17, 64, 4, 8, 1), 2, 17, 1, "k_fwd<true,true,true,1>, one hidden layer")]
    # two column tiles per workgroup: 2·tiles >= 3·256 needs 384 tiles of 16 columns x 32 rows.  The smallest
    # such forward here: T = 24 heads of H = 256 (16 column tiles each, 384 tiles) at M <= 32; T = 24 with
    # A·d = 264 has 17 column tiles (408 tiles): an odd count, the last workgroup of a head has one tile
    + [Probe("tp2_l2_T24_H256", G2(17, 256, 4, 8), 24, 17, 2, "k_fwd<true,false,true,2> hidden layer"),
       Probe("tp2_l1_T24_H256", G2(17, 256, 4, 8), 24, 17, 1, "k_fwd<true,true,true,2> layer 1"),
       Probe("tp2_last_odd_T24", G2(17, 256, 33, 8), 24, 17, 3, "k_fwd<true,false,true,2> 17 column tiles")]
    # layer 0 on its own: fp32 in bf16 mode (the vector kernel at K0 = 32 and 96, the scalar one off alignment)
    + [Probe("l0_own_ns32_H48", G2(32, 48, 4, 8), 2, 17, 0, "k_fwd<true,false,false,1> layer 0 (fp32)"),
       Probe("l0_own_ns96_H64", G2(96, 64, 4, 8), 2, 17, 0, "k_fwd<true,false,false,1> layer 0 (fp32), K0 > 64"),
       Probe("l0_misaligned_ns32_H48", G2(32, 48, 4, 8), 2, 17, 0, "k_fwd<false,false> layer 0, S off alignment",
             aligned=False)]
    # T = 1: no head-major grid -- the 3-D grid (column tiles, heads, row tiles) of every forward kernel
    + [Probe("t1_last_H64_M33", G2(17, 64), 1, 33, 3, "k_fwd<true,false,true,1> last layer, 3-D grid"),
       Probe("t1_last_H32_M7", G2(17, 32), 1, 7, 3, "k_fwd<true,false,true,1> last layer, 3-D grid"),
       Probe("t1_l1_fused_ns17", G2(17, 64, 8, 8), 1, 17, 1, "k_fwd<true,true,true,1> layer 1, 3-D grid"),
       Probe("t1_l2_H64", G2(17, 64, 8, 8), 1, 33, 2, "k_fwd<true,false,true,1> hidden layer, 3-D grid")]
    # K % 32 != 0: the scalar fp32 kernel in bf16 mode
    + [Probe("last_H40_fp32", G2(17, 40), 2, 9, 3, "k_fwd<false,false> (K = 40: fp32)")]
    # the few-row GEMV stays fp32; one row more is a bf16 tile
    + [Probe(f"gemv_M{M}", G2(17, 64, 64, 8), 2, M, 3, "k_fwd_gemv (fp32)" if M <= 4 else "k_fwd<true,false,true,1>")
       for M in (1, 4, 5)]
)


# ---------------------------------------------------------------------------------------------
# backward probes: the layer-1 dX from the GPU's own dZ_1
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BwdProbe:
    id: str
    geo: Geo
    T: int
    B: int
    entry: str                 # "update_all" or "update"
    reaches: str = ""
    seed: int = 0
    max_batch: int = 32


def bwd_rows(p: BwdProbe):
    """i(m), j(m): the input coordinate and the hidden unit of row m (distinct over the rows)."""
    gen = torch.Generator().manual_seed(8000 + p.seed)
    g = p.geo
    assert p.B <= g.n_s <= 64 and p.B <= g.H
    return torch.randperm(g.n_s, generator=gen)[:p.B], torch.randperm(g.H, generator=gen)[:p.B]


def bwd_problem(p: BwdProbe):
    """(heads [T, P], targets [T, P], batch (s, a, r, φ, s1, γ), i, j): S[m] = e_i(m), W_0[:, i(m)] = e_j(m), b_0 = 0,
    the layers above random."""
    from sfx.init import reference_heads

    g = p.geo
    heads, _ = reference_heads(p.T, g.n_s, g.H, g.A, g.d, g.acts, seed=600 + p.seed)
    heads = heads.clone()
    i, j = bwd_rows(p)
    (w0, w1) = g.offsets()[0]
    W0 = torch.zeros(g.H, g.n_s)
    W0[j, i] = 1.0
    heads[:, w0:w1] = W0.reshape(-1)
    heads[:, w1:w1 + g.H] = 0
    gen = torch.Generator().manual_seed(8100 + p.seed)
    S = torch.zeros(p.B, g.n_s)
    S[torch.arange(p.B), i] = 1.0
    S1 = torch.randn(p.B, g.n_s, generator=gen)
    a = torch.randint(0, g.A, (p.B,), generator=gen)
    phi, r = torch.rand(p.B, g.d, generator=gen), torch.rand(p.B, 1, generator=gen)
    target = heads + torch.empty_like(heads).uniform_(-0.05, 0.05, generator=gen)
    return heads, target, (S, a, r, phi, S1, torch.full((p.B,), 0.9)), i, j


def bwd_readout(p: BwdProbe, m_flat: torch.Tensor, i, j):
    """The first moments of one head after the recovery step -> (dZ_1 [B, H], dZ_0 [B, H], db_1 [H]) exactly."""
    g = p.geo
    m_flat = torch.as_tensor(m_flat).detach().cpu().double()
    (a0, a1), (b0, b1) = g.offsets()[0], g.offsets()[1]
    dW0, dW1 = m_flat[a0:a1].view(g.H, g.n_s), m_flat[b0:b1].view(g.H, g.H)
    return dW1[:, j].T.contiguous(), dW0[:, i].T.contiguous(), m_flat[b1:b1 + g.H]


def dx_reference(p: BwdProbe, W1: torch.Tensor, dz1, bf16: bool, ops: Ops = SPEC):
    """(dZ_0 emulation [B, H] in float64, its bound) from dZ_1 [B, H] and layer 1's master weights W1 [H, H]."""
    W = W1.double()
    use_bf = bf16 and (fwd_map(p.geo, p.B)[1] if ops.dx_as_fwd else True)
    dzo, wo = (ops.qdz(dz1), ops.qwdx(W)) if use_bf else (dz1, W)
    dzo, _ = _kg(dzo, wo, ops)
    ref = dzo @ wo
    bound = 2.0 * (W.shape[0] + 1) * U * (dzo.abs() @ wo.abs())
    return ref, bound


def dx_verdict(got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, 1e30, 0.0))
    return float(ratio.max()), got.numel(), int((err > bound).sum())


def db_verdict(dz1, db1):
    """db_1 = sum_m dZ_1[m] within twice the fp32 bound of an M-term sum."""
    ref = dz1.sum(0)
    bound = 2.0 * dz1.shape[0] * U * dz1.abs().sum(0)
    err = (db1 - ref).abs()
    return float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, 1e30, 0.0)).max())


BWD_PROBES: List[BwdProbe] = [
    BwdProbe("mg_ns32_H48", G2(32, 48, 4, 8), 3, 17, "update_all", "k_bwd_mg<true> dx_accum<true,1>"),
    BwdProbe("mg_ns32_H64", G2(32, 64, 4, 8), 3, 32, "update_all", "k_bwd_mg<true> dx_accum<true,1>"),
    BwdProbe("single_ns32_H64", G2(32, 64, 4, 8), 2, 17, "update", "k_bwd<true> role_dx<false,2,8,true>"),
    BwdProbe("single_two_row_tiles", G2(33, 64, 4, 8), 2, 33, "update", "k_bwd<true> role_dx, two row tiles",
             max_batch=64),
    BwdProbe("single_H40", G2(32, 40, 4, 8), 2, 17, "update", "k_bwd<true> role_dx, K % 32 != 0 (fp32 forward)"),
    BwdProbe("all_H40", G2(32, 40, 4, 8), 3, 17, "update_all", "k_bwd_mg<true>, K % 32 != 0 (fp32 forward)"),
    BwdProbe("split_n_H512", G2(17, 512, 4, 8), 2, 8, "update", "k_bwd<true> role_dx split-N"),
    BwdProbe("all_split_n_H512", G2(17, 512, 4, 8), 2, 8, "update_all", "k_bwd<true> role_dx split-N, two heads"),
]


# ---------------------------------------------------------------------------------------------
# composition: two toy whole updates through tests/grad_ref.py's ψ oracle with the emulated Linear
# ---------------------------------------------------------------------------------------------
MID = 2.0 ** -19   # no operand of a bf16 product closer than this (relative to the largest) to a bf16 midpoint


def midpoint_distance(x: torch.Tensor) -> float:
    """Smallest distance of a non-zero element of x from a bf16 rounding midpoint, relative to max |x|."""
    x = x.detach().double().reshape(-1)
    x = x[x != 0]
    if not x.numel():
        return float("inf")
    ulp = 2.0 ** (torch.floor(torch.log2(x.abs())) - 7)
    mid = trunc(x) + torch.sign(x) * ulp / 2
    return float((x - mid).abs().min() / x.abs().max())


def recording_ops():
    """(the specification's Ops, state): state["dist"] is the smallest midpoint_distance of an X or dZ operand."""
    state = {"dist": float("inf")}

    def rq(x):
        state["dist"] = min(state["dist"], midpoint_distance(x))
        return q(x)

    return Ops(qx=rq, qdz=rq), state


@dataclass(frozen=True)
class CompCase:
    id: str
    geo: Geo
    B: int
    seed: int
    T: int = 2


# seeds: the first for which the conditions of comp_oracles hold (`python -m tests.bf16_ref` searches again)
COMP_CASES = [CompCase("fused_td", Geo(17, 32, 3, 8, 1), 4, seed=143),        # A·d = 24: fp32 last-layer dX
              CompCase("plain_last_dx", Geo(17, 32, 9, 16, 1), 3, seed=321)]   # A·d = 144 > 128: a bf16 last dX tile


def comp_oracles(c: CompCase, bf16: bool = True):
    """One sfx_update (GPI) of head T-1 from zero moments -> (problem, ref64, ref32 through the recovery, Info,
    smallest midpoint distance over both emulations)."""
    from tests import grad_ref as GR

    g = c.geo
    pc = GR.PsiCase(c.id, (g.n_s, g.H, g.A, g.d, g.acts), c.B, seed=c.seed, T=c.T)
    st, (b, _) = GR.psi_problem(pc)
    fm, dm = fwd_map(g, c.B, bf16=bf16), dx_map(g, c.T, bf16=bf16)
    ops, state = recording_ops()
    lin = lambda: layerwise(fm, dm, ops)
    g32, info = GR.sf_grads(st, pc.spec, b, c.T - 1, True, make_linear=lin)
    g64, _ = GR.sf_grads(GR.cast(st, F64), pc.spec, GR.cast(b, F64), c.T - 1, True, next_actions=info.next, make_linear=lin)
    return (pc, st, b), g64, {k: GR.through_moments(v) for k, v in g32.items()}, info, state["dist"]


if __name__ == "__main__":
    import dataclasses
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "deep-successor-features-for-transfer_amd"))
    for c in COMP_CASES:
        for seed in range(2000):
            _, _, _, info, dist = comp_oracles(dataclasses.replace(c, seed=seed))
            if info.ok() and dist > MID:
                print(c.id, "seed", seed, "midpoint distance", dist, flush=True)
                break
        else:
            raise SystemExit(f"no seed for {c.id}")


# ---------------------------------------------------------------------------------------------
# sfx_update's own forward launches (three groups of one, one and T heads: never the head-major grid)
# ---------------------------------------------------------------------------------------------
# The last layer is under test, B <= A rows take distinct actions a_m, and the step is the recovery step, so
#   db_last[a_m d + k] = dZ_last[m, a_m d + k] = c (ψ(s)[m, a_m, k] - φ[m, k] - γ ψ⁻(s1)[m, a'_m, k]),  c = 2 / (B A d),
# a single term.  With φ = 0, γ = 0 that is c ψ(s)[m, a_m] of the online group; with s = 0 and a zero last bias in the
# online head (ψ(s) = 0 exactly), φ = 0, γ = 1 it is -c ψ⁻(s1)[m, a'_m] of the target group, a' read back from the call.
# c is a power of two at B·A·d = 2048 (exact); elsewhere the scaling's roundings (the factor, its product) are allowed
# for by UPD_EXTRA ulps of the value on top of the product's bound.
UPD_EXTRA = 4
UPD_PROBES: List[Probe] = [
    Probe("upd_A16_B16", G2(17, 64, 16, 8), 3, 16, 3, "k_fwd<true,false,true,1> last layer, update's groups (c = 2^-10)"),
    Probe("upd_A17_B17", G2(17, 64, 17, 8), 3, 17, 3, "k_fwd<true,false,true,1> last layer, update's groups"),
    Probe("upd_T1_A17_B7", G2(17, 32, 17, 8), 1, 7, 3, "k_fwd<true,false,true,1> last layer, update at T = 1"),
]


def upd_scale(p: Probe) -> float:
    return 2.0 / (p.M * p.geo.A * p.geo.d)


def upd_verdict(p: Probe, m_flat, acts_taken, acts_read, z, bound, sign: float):
    """The first moments of the updated head -> (worst error / bound, elements, misses) of ψ[m, acts_read[m], :]
    against z, bound [M, A·d]; row m's action acts_taken[m] says where its dZ sits in db_last."""
    g = p.geo
    w1 = g.offsets()[-1][1]
    db = torch.as_tensor(m_flat).detach().cpu().double()[w1:w1 + g.A * g.d].view(g.A, g.d)
    got = sign * db[acts_taken] / upd_scale(p)                                   # [M, d]
    rows = torch.arange(p.M)
    zz, bb = z.view(p.M, g.A, g.d)[rows, acts_read], bound.view(p.M, g.A, g.d)[rows, acts_read]
    n = p.M * g.A * g.d
    if n & (n - 1):
        bb = bb + UPD_EXTRA * U * zz.abs()
    err = (got - zz).abs()
    return float((err / bb.clamp(min=1e-300)).max()), got.numel(), int((err > bb).sum())
