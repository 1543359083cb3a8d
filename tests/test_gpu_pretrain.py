"""The φ pre-training handle on the GPU (include/sfx.h sfx_pre_*, csrc/sfx_pre.h; sfdqn_phi.py:90-123, :800-873):
one update against the float32 restatement, gradient values and the Adam step against float64, a 60-update
trajectory under its float64 budget, the forward, the limits, the driver on the real reference's losses, and a
checkpoint round trip.  tests/pretrain_ref.py is the restatement, tests/grad_ref.py and tests/adam_ref.py the bounds.

Shapes: the smallest at which the kernels can still go wrong.  (4, 12, 128/256) is the reference's own, n_in = 9 odd;
24/40 exercises the tile tails; 16/16 at n_s = 17 a wider odd input; one and four hidden layers; (31, 64, 256/256) sits
at every limit.  B in {1, 5, 32, 64} covers one to four 16-row tiles and their tails.  T = 3.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adam_ref as AR
from tests import grad_ref as GR
from tests import pretrain_ref as PR
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

T = 3
A_COUNT = 9
SHAPES = [(4, 12, (128, 256)), (4, 12, (24, 40)), (17, 8, (16, 16)), (4, 12, (256,)), (4, 12, (8, 8, 8, 8)),
          (31, 64, (256, 256))]
BS = (1, 5, 32, 64)
OFF = 11   # step-count offset between the rows and the net, so that none can be taken for another
_ids = lambda s: f"ns{s[0]}-d{s[1]}-h" + "x".join(map(str, s[2]))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


# ---------------------------------------------------------------------------------------------------------------
# problems (CPU; shared with tests/test_pretrain_golden.py)
# ---------------------------------------------------------------------------------------------------------------
def kink_free(e: PR.RefEngine, b) -> PR.RefEngine:
    """ReLU biases nudged off the rows' zero crossings (tests/grad_ref.py clear_kinks), so that float32 and float64
    gradients do not differ by a whole unit's contribution."""
    flat = e.flat.clone()
    GR.clear_kinks(flat, e.dims, ("relu",) * (len(e.dims) - 1) + (None,), PR.inputs(b[0], b[1], b[3], e.dtype))
    e.load(flat)
    return e


def case(shape, B, seed=0, w_scale=None):
    n_s, d, hidden = shape
    e = PR.problem(n_s, d, T, hidden, 5000 + seed)
    gen = torch.Generator().manual_seed(6000 + seed)
    b = PR.batch(n_s, A_COUNT, B, gen)
    if w_scale is not None:
        for t in range(T):
            e.load_w(t, e.w[t] * (w_scale / 0.01))
    return kink_free(e, b), b


def load_state(e: PR.RefEngine, k0: int, task: int, b, seed: int):
    """Loaded moments at the scale of each group's gradient (adam_ref.loaded_moments), the net at step k0 and row
    t at k0 + OFF (t + 1); k0 = 0 keeps the net's moments zero, the rows' stay loaded."""
    e64 = e.clone(torch.float64)
    gf = e64.grads(task, *b)[1]
    ms, vs, off = [], [], 0
    for o, i in e.dims:
        for n in (o * i, o):
            m, v = AR.loaded_moments(gf[off:off + n], k0, seed + off)
            ms.append(m), vs.append(v)
            off += n
    e.load_adam(torch.cat(ms), torch.cat(vs), k0)
    for t in range(e.T):
        gw = e64.grads(t, *b)[2]
        m, v = AR.loaded_moments(gw, k0 + OFF * (t + 1), seed + 97 * (t + 1))
        e.load_w(t, e.w[t], m, v, k0 + OFF * (t + 1))
    return e


def net_consts(hp: AR.HP, step: int):
    return AR.consts(hp.lr_psi, hp.wd_psi, hp.betas, hp.eps, step)


def row_consts(hp: AR.HP, step: int):
    return AR.consts(hp.lr_w, hp.wd_w, hp.betas, hp.eps, step)


def set_hp(e, hp: AR.HP):
    e.set_adam(hp.lr_psi, hp.wd_psi, hp.lr_w, hp.wd_w, betas=hp.betas, eps=hp.eps)


def adam_case(hp: AR.HP, k0: int, shape=SHAPES[0], B=32, task=1, mutant=None):
    """(restatement, its mutant or None, batch, task, k0) of one measured run of the Adam test."""
    e, b = case(shape, B, seed=3)
    load_state(e, k0, task, b, 40 + k0)
    set_hp(e, hp)
    return e, (e.clone(mutant=mutant) if mutant else None), b, task, k0


N_TRAJ, PER_TASK = 60, 5


def trajectory_problem(shape=SHAPES[0], B=32):
    n_s, d, hidden = shape
    e = PR.problem(n_s, d, T, hidden, 5100)
    gen = torch.Generator().manual_seed(6100)
    return e, [PR.batch(n_s, A_COUNT, B, gen) for _ in range(N_TRAJ)], PR.cycle_order(T, N_TRAJ, PER_TASK)


# ---------------------------------------------------------------------------------------------------------------
# engine helpers
# ---------------------------------------------------------------------------------------------------------------
def engine_of(e: PR.RefEngine, max_batch=64):
    from sfx.pretrain import PreEngine

    eng = PreEngine(e.n_s, e.d, e.T, e.hidden, max_batch=max_batch, device="cuda:0")
    hp = e.adam_hp
    eng.set_adam(hp["lr_phi"], hp["wd_phi"], hp["lr_w"], hp["wd_w"], hp["betas"], hp["eps"])
    push(eng, e)
    return eng


def push(eng, e: PR.RefEngine):
    eng.load(e.flat)
    eng.load_adam(e.m, e.v, e.step)
    for t in range(e.T):
        eng.load_w(t, e.w[t], e.wm[t], e.wv[t], e.wstep[t])


def rows_untouched(eng, e: PR.RefEngine, task: int):
    for t in range(e.T):
        if t == task:
            continue
        w, m, v, step = eng.get_w(t)
        assert torch.equal(w, e.w[t]) and torch.equal(m, e.wm[t]) and torch.equal(v, e.wv[t]), f"row {t} changed"
        assert step == e.wstep[t], f"row {t}: step {step}, loaded {e.wstep[t]}"


def group_slices(e: PR.RefEngine):
    out, off = [], 0
    for l, (o, i) in enumerate(e.dims):
        out += [(f"W{l}", off, off + o * i), (f"b{l}", off + o * i, off + o * i + o)]
        off += o * i + o
    return out


# ---------------------------------------------------------------------------------------------------------------
# 1. one update from an identical loaded state
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_one_update(shape, B):
    task = 1
    e, b = case(shape, B)
    load_state(e, 3, task, b, 17)
    eng = engine_of(e)
    loss = float(eng.update(task, *b))
    ref = e.clone()
    want = float(ref.update(task, *b))
    print(f"loss {loss!r} restatement {want!r}")
    np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-7)
    rows_untouched(eng, e, task)
    assert eng.get_adam()[2] == 4 and eng.get_w(task)[3] == 3 + OFF * (task + 1) + 1
    assert not torch.equal(eng.get(), e.flat) and not torch.equal(eng.get_w(task)[0], e.w[task])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. gradient values
# ---------------------------------------------------------------------------------------------------------------
def recover(eng, e: PR.RefEngine, task, b):
    """The recovery run of tests/test_gpu_adam.py: zero moments, every lr and decay 0, betas (0, β2): the first
    moments read back are the kernel's gradients bit for bit, and no parameter moves."""
    z = e.clone()
    z.load_adam(torch.zeros(e.P), torch.zeros(e.P), 0)
    for t in range(e.T):
        z.load_w(t, e.w[t], None, None, 0)
    push(eng, z)
    eng.set_adam(0.0, 0.0, 0.0, 0.0, betas=(0.0, 0.999), eps=1e-8)
    eng.update(task, *b)
    gf, gw = eng.get_adam()[0], eng.get_w(task)[1]
    assert torch.equal(eng.get(), e.flat) and torch.equal(eng.get_w(task)[0], e.w[task]), "a parameter moved at lr 0"
    rows_untouched(eng, z, task)
    return gf, gw


# every shape at one, two and four row tiles with their tails; one row at the reference's shape (with one row a
# narrow net can have a whole layer dead, and the oracle's gradient is then identically zero)
GRAD_CASES = [(s, B) for s in SHAPES for B in (5, 32, 64)] + [(SHAPES[0], 1)]


@pytest.mark.parametrize("shape,B", GRAD_CASES, ids=lambda x: _ids(x) if isinstance(x, tuple) else f"B{x}")
def test_gradient_values(shape, B):
    task = 2
    e, b = case(shape, B, seed=1)
    e64 = e.clone(torch.float64)
    _, gf64, gw64, relu_min = e64.grads(task, *b, relu_min=True)
    _, gf32, gw32, _ = e.grads(task, *b)
    assert relu_min >= 0.5 * GR.MARGIN, f"a ReLU pre-activation at {relu_min:.2e}"
    eng = engine_of(e)
    gf, gw = recover(eng, e, task, b)
    gf2, gw2 = recover(eng, e, task, b)
    assert torch.equal(gf, gf2) and torch.equal(gw, gw2), "two runs from the same state differ"
    for name, lo, hi in group_slices(e):
        GR.grad_close(f"pre {_ids(shape)} B{B} {name}", gf[lo:hi], gf64[lo:hi], gf32[lo:hi])
    GR.grad_close(f"pre {_ids(shape)} B{B} w", gw, gw64, gw32)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. the Adam step
# ---------------------------------------------------------------------------------------------------------------
ADAM_CASES = [(hp, k0, SHAPES[0], 32) for hp in AR.NON_DEFAULT for k0 in AR.K0S] + [(AR.HP_SETS[1], 3, SHAPES[1], 5)]


@pytest.mark.parametrize("hp,k0,shape,B", ADAM_CASES, ids=lambda x: getattr(x, "id", None) or (
    _ids(x) if isinstance(x, tuple) else str(x)))
def test_adam_step(hp, k0, shape, B):
    e, _, b, task, _ = adam_case(hp, k0, shape, B)
    eng = engine_of(e)
    gf, gw = recover(eng, e, task, b)
    gf2, gw2 = recover(eng, e, task, b)
    assert torch.equal(gf, gf2) and torch.equal(gw, gw2)
    push(eng, e)
    set_hp(eng, hp)
    eng.update(task, *b)
    m, v, step = eng.get_adam()
    assert step == k0 + 1
    w, wm, wv, wstep = eng.get_w(task)
    k_row = k0 + OFF * (task + 1)
    assert wstep == k_row + 1
    rows_untouched(eng, e, task)
    path = f"pre_update {hp.id} k0={k0} {_ids(shape)} B{B}"
    p = eng.get()
    c = net_consts(hp, k0 + 1)
    for name, lo, hi in group_slices(e):
        ex = AR.expect(e.flat[lo:hi], gf[lo:hi], e.m[lo:hi], e.v[lo:hi], c)
        AR.check(path, name, dict(p=p[lo:hi], m=m[lo:hi], v=v[lo:hi]), ex)
    ex = AR.expect(e.w[task], gw, e.wm[task], e.wv[task], row_consts(hp, k_row + 1))
    AR.check(path, "w", dict(p=w, m=wm, v=wv), ex)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. trajectory
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", [(SHAPES[0], 32), (SHAPES[1], 5)], ids=lambda x: _ids(x) if isinstance(x, tuple) else f"B{x}")
def test_trajectory_budget_vs_float64(shape, B):
    """60 updates over T = 3 in the reference's cycle order (5 per task and cycle).  Per group the GPU's
    max |p - p64| is at most 2x the float32 restatement's plus one fp32 ulp of the group's largest magnitude; every
    loss within 1e-5 relative of float64's (tests/pretrain_ref.py budget_check)."""
    e, batches, order = trajectory_problem(shape, B)
    e64 = e.clone(torch.float64)
    ref32 = e.clone()
    l32, l64 = PR.run(ref32, batches, order), PR.run(e64, batches, order)
    eng = engine_of(e)
    losses = torch.zeros(N_TRAJ, device="cuda:0")
    for j, (t, b) in enumerate(zip(order, batches)):
        eng.update(t, *b, out=losses[j:j + 1])
    got = PR.split_groups(e.dims, eng.get(), torch.stack([eng.get_w(t)[0] for t in range(T)]))
    assert eng.get_adam()[2] == N_TRAJ and [eng.get_w(t)[3] for t in range(T)] == [order.count(t) for t in range(T)]
    PR.budget_check(f"pre_update {_ids(shape)} B{B}", got, losses.cpu(), ref32, l32, e64, l64)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. the forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_features(shape):
    task = 0
    e, b = case(shape, 64, seed=2, w_scale=1.0)
    S, a, r, S1 = b
    eng = engine_of(e)
    phi64 = e.clone(torch.float64).features(S, a, S1)
    phi32 = e.features(S, a, S1)
    for B in (5, 32, 64):
        got = eng.features(S[:B], a[:B], S1[:B])
        for row in range(B):
            one = eng.features(S[row:row + 1], a[row:row + 1], S1[row:row + 1])
            assert torch.equal(got[row:row + 1], one), f"B = {B}: row {row} is not the one-row call's"
        GR.grad_close(f"pre_features {_ids(shape)} B{B}", got, phi64[:B], phi32[:B])
        # the φ that the next update's loss implies: (d + B + 4) roundings of 2^-24 on a loss whose terms do not
        # cancel (r in [0.5, 1.5], the rows' ŷ of either sign) stay below 1e-5
        phi = got.cpu().double()
        rr = r[:B] + 0.5
        want = float(((rr.double() - phi @ e.w[task].double()) ** 2).mean())
        push(eng, e)
        loss = float(eng.update(task, S[:B], a[:B], rr, S1[:B]))
        np.testing.assert_allclose(loss, want, rtol=1e-5)
        push(eng, e)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. limits
# ---------------------------------------------------------------------------------------------------------------
def test_limits():
    from sfx._lib import lib

    def create(n_s=4, d=12, T_=3, hidden=(128, 256), n_hidden=None, max_batch=32, null_hidden=False, null_out=False):
        h = C.c_void_p()
        hid = (C.c_int * max(1, len(hidden)))(*hidden)
        rc = lib.sfx_pre_create(None if null_out else C.byref(h), n_s, d, T_, None if null_hidden else hid,
                                len(hidden) if n_hidden is None else n_hidden, max_batch)
        return rc, lib.sfx_last_error().decode(), h

    for kw, word in ((dict(n_s=32), "n_in"), (dict(n_s=0), "n_in"), (dict(hidden=()), "hidden layers"),
                     (dict(hidden=(8,) * 5), "hidden layers"), (dict(hidden=(128, 257)), "hidden width"),
                     (dict(hidden=(0, 8)), "hidden width"), (dict(d=65), "d <= 64"), (dict(d=0), "d <= 64"),
                     (dict(max_batch=65), "max_batch"), (dict(max_batch=0), "max_batch"), (dict(T_=0), "T >= 1"),
                     (dict(null_hidden=True), "null"), (dict(null_out=True), "null")):
        rc, msg, h = create(**kw)
        assert rc == -1 and word in msg and ("limit" in msg or "null" in msg), (kw, rc, msg)
        assert not h.value
    rc, _, h = create()
    assert rc == 0
    e, b = case(SHAPES[0], 32)
    S, a, r, S1 = (x.to("cuda:0") for x in b)
    loss, phi = torch.zeros(1, device="cuda:0"), torch.zeros(32, 12, device="cuda:0")
    ptr = lambda t: t.data_ptr()
    upd = lambda task=0, S_=ptr(S), a_=ptr(a), r_=ptr(r), S1_=ptr(S1), B=32, out=ptr(loss): \
        lib.sfx_pre_update(h, task, S_, a_, r_, S1_, B, out)
    fea = lambda S_=ptr(S), a_=ptr(a), S1_=ptr(S1), B=32, out=ptr(phi): lib.sfx_pre_features(h, S_, a_, S1_, B, out)
    for call, word in ((lambda: upd(task=-1), "task"), (lambda: upd(task=3), "task"), (lambda: upd(B=0), "max_batch"),
                       (lambda: upd(B=33), "max_batch"), (lambda: upd(S_=None), "null"), (lambda: upd(a_=None), "null"),
                       (lambda: upd(r_=None), "null"), (lambda: upd(S1_=None), "null"), (lambda: upd(out=None), "null"),
                       (lambda: fea(B=0), "max_batch"), (lambda: fea(B=33), "max_batch"), (lambda: fea(S_=None), "null"),
                       (lambda: fea(out=None), "null"), (lambda: lib.sfx_pre_update(None, 0, ptr(S), ptr(a), ptr(r),
                                                                                   ptr(S1), 32, ptr(loss)), "null"),
                       (lambda: lib.sfx_pre_load(h, None), "null"),
                       (lambda: lib.sfx_pre_load_w(h, 3, None, None, None, 0), "null")):
        assert call() == -1
        assert word in lib.sfx_last_error().decode(), lib.sfx_last_error()
    # no launch was made: the step counts on the device are where they started
    m, v, step = np.empty(lib.sfx_pre_numel(h), np.float32), np.empty(lib.sfx_pre_numel(h), np.float32), C.c_int(-1)
    from sfx._lib import fptr

    assert lib.sfx_pre_get_adam(h, fptr(m), fptr(v), C.byref(step)) == 0 and step.value == 0
    assert not m.any() and not v.any() and float(loss) == 0.0
    assert lib.sfx_pre_destroy(h) == 0


# ---------------------------------------------------------------------------------------------------------------
# 7. the driver
# ---------------------------------------------------------------------------------------------------------------
def test_driver_on_the_reference_recipe(golden):
    """sfx.pretrain.pre_train on the recipe of tests/golden/pretrain_phi.npz.  The losses are held to the trajectory
    budget (1e-5 relative of the float64 restatement fed the recorded transitions) step by step; the real
    reference's recorded losses are held to the same budget, which ties the two together."""
    from sfx import pretrain
    from tests.test_pretrain_golden import recipe, seeded_engine

    g = golden("pretrain_phi")
    c = recipe(g)
    e64 = seeded_engine(c, PR.RefEngine(c["n_s"], c["d"], c["T"], c["hidden"], torch.float64))
    S, a, r, S1 = (torch.from_numpy(g[k]) for k in ("S", "a", "r", "S1"))
    nb = int(g["idx"].shape[1])
    l64 = []
    for j in range(nb - 1, S.shape[0]):
        idx = torch.from_numpy(g["idx"][j + 1 - nb])
        l64.append(float(e64.update((j // c["n"]) % c["T"], S[idx], a[idx], r[idx], S1[idx])))
    tasks = [PR.SynthTask(c["n_s"], c["A"], c["d"], t) for t in range(c["T"])]
    PR.seed_all(c["seed"])
    phi, losses = pretrain.pre_train(tasks, c["n"], c["cycles"], hidden=c["hidden"], device="cuda:0")
    states = PR.rng_states()
    assert len(losses) == len(l64) == len(g["losses"]) and isinstance(losses[0], float)
    for j, (x, y, z) in enumerate(zip(losses, l64, g["losses"])):
        print(j, x, y, float(z))
    np.testing.assert_allclose(g["losses"], l64, rtol=PR.LOSS_RTOL)
    np.testing.assert_allclose(losses, l64, rtol=PR.LOSS_RTOL)
    for k, v in states.items():
        assert np.array_equal(np.asarray(v), g[k]), f"{k}: the loop drew from this generator in another order"
    s, s1, act = S[:3], S1[:3], a[:3]
    want = phi(s, act, s1)
    assert want.device.type == "cuda" and tuple(want.shape) == (3, c["d"])
    assert torch.equal(phi(s[0], act[0], s1[0]), want[:1])                       # 0-d action, 1-d states
    assert torch.equal(phi(s, act.float(), s1), want)                            # tsfdqn_phi.py's float32 action
    assert torch.equal(phi(s.cuda(), act.unsqueeze(1).cuda(), s1.cuda()), want)  # device tensors, a [B, 1]
    assert phi.set_eval() is None
    mod = phi.to_module()
    ref_shape = pretrain.PhiModule(c["n_s"], c["d"], (128, 256))
    ref_shape.load_state_dict(mod.state_dict())
    np.testing.assert_allclose(ref_shape(s, act, s1).detach().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6)
    phi.engine.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. checkpoint
# ---------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(tmp_path):
    from sfx import checkpoint

    e, batches, order = trajectory_problem(SHAPES[1], 5)
    eng = engine_of(e)
    eng.set_adam(7e-4, 2e-2, 1.3e-3, 0.6, betas=(0.8, 0.9992), eps=1e-3)
    for t, b in list(zip(order, batches))[:7]:     # two tasks trained, the third's Adam still without state
        eng.update(t, *b)
    path = str(tmp_path / "pre.pt")
    checkpoint.save_pre(eng, path)
    ck = torch.load(path, weights_only=True)
    assert list(ck["phi_model"]) == [f"_model.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    assert ck["rows"][2]["optim"]["state"] == {} and int(ck["phi_optim"]["state"][0]["step"]) == 7
    other = engine_of(PR.problem(e.n_s, e.d, T, e.hidden, 1))
    checkpoint.load_pre(other, path)
    read = lambda x: (x.get(), *x.get_adam(), *[y for t in range(T) for y in x.get_w(t)])
    for u, w in zip(read(eng), read(other)):
        assert torch.equal(u, w) if torch.is_tensor(u) else u == w
    assert other.adam_hp == eng.adam_hp
    t, b = order[7], batches[7]
    assert float(eng.update(t, *b)) == float(other.update(t, *b))
    for u, w in zip(read(eng), read(other)):
        assert torch.equal(u, w) if torch.is_tensor(u) else u == w
    with pytest.raises(ValueError, match="geometry"):
        checkpoint.load_pre(engine_of(PR.problem(e.n_s, e.d, T, (24, 44), 1)), path)
    eng.close(), other.close()
