"""The φ pre-training phase on the CPU: tests/pretrain_ref.py (the torch restatement of sfdqn_phi.py:90-123 and
:800-873) and the loop sfx.pretrain.pre_train against golden vectors from the real reference
(tests/golden/pretrain_phi.npz, tools/gen_pretrain_golden.py), the drop-in binding of the two single-file
modules, and the float64 budget of the GPU trajectory test held against the float32 restatement and three mutants.

Tolerances of the restatement as in tests/test_phi_test_golden.py: losses to 1e-5 relative, the final parameters by
params_close with lr_steps = lr · k and no entry allowed out."""
import sys
import textwrap

import numpy as np
import pytest
import torch

from tests import pretrain_ref as PR
from tests.test_gpu_engine import params_close, rel_close


def recipe(g):
    return dict(n_s=int(g["n_s"]), A=int(g["A"]), d=int(g["d"]), T=int(g["T"]), n=int(g["n"]),
                cycles=int(g["cycles"]), seed=int(g["seed"]), hidden=tuple(int(h) for h in g["hidden"]))


def seeded_engine(c, engine):
    """The initial state pre_train builds from the recipe's seeds (PhiFunction's init, then each row's draws)."""
    from sfx.pretrain import PhiModule, pack_module

    PR.seed_all(c["seed"])
    engine.load(pack_module(PhiModule(c["n_s"], c["d"], c["hidden"])))
    for t in range(c["T"]):
        torch.nn.Linear(c["d"], 1, bias=False)
        engine.load_w(t, torch.Tensor(1, c["d"]).uniform_(-0.01, 0.01).reshape(-1))
    return engine


def test_restatement_reproduces_the_reference(golden):
    g = golden("pretrain_phi")
    c = recipe(g)
    e = seeded_engine(c, PR.RefEngine(c["n_s"], c["d"], c["T"], c["hidden"], torch.float32))
    S, a, r, S1 = (torch.from_numpy(g[k]) for k in ("S", "a", "r", "S1"))
    losses, nb = [], int(g["idx"].shape[1])
    for j in range(S.shape[0]):
        if j + 1 < nb:
            continue
        idx = torch.from_numpy(g["idx"][j + 1 - nb])
        assert int(idx.max()) <= j
        losses.append(float(e.update((j // c["n"]) % c["T"], S[idx], a[idx], r[idx], S1[idx])))
    assert len(losses) == len(g["losses"]) == 129
    rel_close(losses, g["losses"], rtol=1e-5, atol=1e-9)
    params_close(e.get(), g["phi"], 1e-3 * len(losses), max_bad_frac=0.0)
    assert e.step == 129 and sum(e.wstep) == 129 and e.wstep[0] != e.wstep[1]


def test_pre_train_consumes_the_rngs_in_the_reference_order(golden):
    from sfx import pretrain

    g = golden("pretrain_phi")
    c = recipe(g)
    tasks = [PR.SynthTask(c["n_s"], c["A"], c["d"], t) for t in range(c["T"])]
    eng = PR.RefEngine(c["n_s"], c["d"], c["T"], c["hidden"], torch.float32)
    PR.seed_all(c["seed"])
    phi, losses = pretrain.pre_train(tasks, c["n"], c["cycles"], hidden=c["hidden"], engine=eng)
    states = PR.rng_states()
    assert isinstance(phi, pretrain.LearntPhi) and isinstance(losses, list) and isinstance(losses[0], float)
    rel_close(losses, g["losses"], rtol=1e-5, atol=1e-9)
    params_close(eng.get(), g["phi"], 1e-3 * len(losses), max_bad_frac=0.0)
    for k, v in states.items():
        assert np.array_equal(np.asarray(v), g[k]), f"{k}: the loop drew from this generator in another order"
    # the frozen net, in every call form of PhiFunction.forward
    s, s1 = torch.from_numpy(g["S"][:3]), torch.from_numpy(g["S1"][:3])
    a = torch.from_numpy(g["a"][:3])
    want = phi(s, a, s1)
    assert tuple(want.shape) == (3, c["d"])
    # (torch's CPU GEMM is not row-for-row identical across batch sizes; that promise is the library's, on the GPU)
    np.testing.assert_allclose(phi(s[0], a[0], s1[0]).numpy(), want[:1].numpy(), rtol=1e-6, atol=1e-7)
    assert torch.equal(phi(s, a.float(), s1), want) and torch.equal(phi(s, a.unsqueeze(1), s1), want)
    mod = phi.to_module()
    assert [n for n, _ in mod.named_parameters()] == [f"_model.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    np.testing.assert_allclose(mod(s, a, s1).detach().numpy(), want.numpy(), rtol=1e-6, atol=1e-7)
    assert phi.set_eval() is None


def test_drop_in_binds_the_single_file_modules(tmp_path):
    from sfx import dropin
    from sfx.dropin import bind

    assert "sfdqn_phi" in dropin.BOUND and "tsfdqn_phi" in dropin.BOUND
    assert "sfdqn_phi" in dropin.__doc__ and "tsfdqn_phi" in dropin.__doc__
    stand_in = textwrap.dedent("""
        WHO = 'user'
        class PhiFunction:
            pass
        class {cls}:
            def pre_train(self, train_tasks, n_samples_pre_train, n_cycles=5):
                return 'user pre_train'
            def train_agent(self):
                return 'user train'
        """)
    (tmp_path / "sfdqn_phi.py").write_text(stand_in.format(cls="SFDQN"))
    (tmp_path / "tsfdqn_phi.py").write_text(stand_in.format(cls="TSFDQN"))

    def forget():
        sys.meta_path[:] = [f for f in sys.meta_path if not isinstance(f, dropin._Finder)]
        for name in ("sfdqn_phi", "tsfdqn_phi"):
            sys.modules.pop(name, None)

    forget()
    sys.path.insert(0, str(tmp_path))
    try:
        dropin.install()
        import sfdqn_phi
        import tsfdqn_phi

        for cls in (sfdqn_phi.SFDQN, tsfdqn_phi.TSFDQN):
            assert cls.pre_train is bind.lib_pre_train and cls.pre_train.__sfx_bound__
            assert cls().train_agent() == "user train"       # everything else stays the user's
        assert sfdqn_phi.WHO == "user" and sfdqn_phi.PhiFunction.__module__ == "sfdqn_phi"
    finally:
        sys.path.remove(str(tmp_path))
        forget()
    bind.patch("sfdqn_phi", type(sys)("empty"))     # a module without the class is left alone


# ---------------------------------------------------------------------------------------------------------------
# the float64 budget (tests/pretrain_ref.py budget_check) on the GPU trajectory test's problem
# ---------------------------------------------------------------------------------------------------------------
def test_float64_budget_passes_the_restatement_and_catches_the_mutants():
    from tests.test_gpu_pretrain import trajectory_problem

    e32, batches, order = trajectory_problem()
    e64 = e32.clone(torch.float64)
    ref32 = e32.clone()
    l32, l64 = PR.run(ref32, batches, order), PR.run(e64, batches, order)
    PR.budget_check("float32 restatement", ref32.groups(), l32, ref32, l32, e64, l64)
    for name in PR.MUTANTS:
        mut = e32.clone(mutant=name)
        lm = PR.run(mut, batches, order)
        with pytest.raises(AssertionError):
            PR.budget_check(name, mut.groups(), lm, ref32, l32, e64, l64)


def test_adam_lr_shows_a_stale_layer0_gradient():
    """The measured run of the GPU Adam test: a dW_0 taken from already stepped upper layers leaves
    tests/adam_ref.py's bound on p', m' and v' of the first layer at that run's learning rates."""
    from tests import adam_ref as AR
    from tests.test_gpu_pretrain import adam_case, net_consts

    for hp in AR.NON_DEFAULT:
        ref, mut, b, task, k0 = adam_case(hp, 3, mutant="stale_dw0")
        p0, m0, v0 = ref.flat.clone(), ref.m.clone(), ref.v.clone()
        g = ref.grads(task, *b)[1]      # the gradient the float32 step itself uses, as the GPU test recovers its own
        n0 = ref.dims[0][0] * (ref.dims[0][1] + 1)
        e = AR.expect(p0[:n0], g[:n0], m0[:n0], v0[:n0], net_consts(hp, k0 + 1))
        ref.update(task, *b)
        mut.update(task, *b)
        ok = AR.worst(dict(p=ref.flat[:n0], m=ref.m[:n0], v=ref.v[:n0]), e)
        assert max(r for r, _ in ok.values()) <= 1.0, (hp.id, ok)
        w = AR.worst(dict(p=mut.flat[:n0], m=mut.m[:n0], v=mut.v[:n0]), e)
        assert max(r for r, _ in w.values()) > 1.0, (hp.id, w)
