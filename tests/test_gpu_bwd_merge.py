"""The merged last backward launch (run_bwd): the layer-0 dW tiles of the many-head
callers, 16 columns wide, compute their own 16 columns of dZ_0 -- one dX tile of layer 1, which a
launch of its own used to run -- so a round has one backward launch fewer.

The tile does role_dx's arithmetic (same split of N over waves and lane groups, same MFMA k order,
same wave-order reduction, same act_bwd), so everything must be IDENTICAL to SFX_BWD_MERGE=0, which
keeps the separate launch: torch.equal on heads, moments, step counts and every action.  Shapes
where the merged form does not apply (more than one 32-row tile, a split-N dX) keep the old
sequence whatever the switch says and still match the oracle.
"""
import pytest
import torch

from oracle import ref_cpu as R
from tests.conftest import gpu_available
from tests.test_gpu_runner import check_state, make, replay_with_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


def run_loop(monkeypatch, merge, spec, T, B, n, ev=7, force=-1, precision=None, max_batch=None, record_oracle=False):
    """n native-runner steps (round skipping and look-ahead on, as by default; a target sync every
    `ev` updates) on a handle created with SFX_BWD_MERGE=merge; everything a step leaves behind, and
    the engine's skip statistics as they stood when the run closed it."""
    from sfx.runner import NativeEnvLoop

    monkeypatch.setenv("SFX_BWD_MERGE", merge)
    eng, st = make(spec, T, ev, max_batch=max_batch or B)
    if precision:
        eng.set_precision(precision)
    if force >= 0:
        eng.debug_force_rerun(force)
    loop = NativeEnvLoop(eng, batch=B, capacity=300, gamma=0.9, epsilon=0.2, alpha_w=0.05, episode_len=11, seed=9)
    loop.prefill(B + 8)
    loop.set_task(1)
    loop.record(n)
    loop.run(n)
    recs = loop.records()
    final = loop.action()
    if record_oracle:
        replay_with_oracle(st, spec, recs, 0.05, ev, final)
        check_state(eng, st, T, n)
    out = dict(heads=torch.stack([eng.get_head(t, 0) for t in range(T)]),
               targets=torch.stack([eng.get_head(t, 1) for t in range(T)]),
               moms=[eng.get_adam(t) for t in range(T)],
               actions=[(r["c"], r["a_greedy"]) for r in recs], final=final, stats=loop.stats())
    loop.close()
    out["skips"] = eng.skip_stats()
    eng.close()
    return out


def assert_identical(x, y):
    assert x["actions"] == y["actions"] and x["final"] == y["final"]
    assert torch.equal(x["heads"], y["heads"]) and torch.equal(x["targets"], y["targets"])
    for (ma, va, sa), (mb, vb, sb) in zip(x["moms"], y["moms"]):
        assert torch.equal(ma, mb) and torch.equal(va, vb) and sa == sb


def bwd_launches(monkeypatch, merge, spec, T, B, max_batch=None):
    """(backward launches of one update_all, Linear layers of the net)."""
    monkeypatch.setenv("SFX_BWD_MERGE", merge)
    eng, _ = make(spec, T, 1000, max_batch=max_batch or B)
    gen = torch.Generator().manual_seed(3)
    s, s1 = torch.randn(B, spec.n_s, generator=gen), torch.randn(B, spec.n_s, generator=gen)
    a = torch.randint(0, spec.A, (B,), generator=gen)
    phi = torch.rand(B, spec.d, generator=gen)
    eng.prof_enable(True)
    eng.prof_reset()
    eng.update_all(s.cuda(), a.cuda(), phi.cuda(), s1.cuda(), torch.full((B,), 0.9).cuda())
    eng.synchronize()
    n = eng.prof_collect()["bwd"][0]
    eng.prof_enable(False)
    eng.close()
    return n, len(spec.acts) + 2


CASES = {
    # ragged last layer-0 tile (columns 32..39), a half-valid dX sub-tile, dZ_1 rows by dword loads
    "ragged-h40-b7": dict(spec=R.Spec(17, 40, 7, 8, ("relu", "relu")), T=3, B=7),
    # H = 16: the second dX sub-tile of the only layer-0 tile does not exist
    "single-subtile-h16": dict(spec=R.Spec(4, 16, 7, 8, ("relu", "relu")), T=3, B=32),
    # one hidden layer: TD + dX_2, then the merged launch with the loss tail; dZ_1 rows as float4
    "vector-one-hidden": dict(spec=R.Spec(17, 64, 7, 8, ("relu",)), T=3, B=32),
    # T A > 256: the TD target is a launch of its own (k_tdgw), the tail rides the first backward
    "unfused-td-t40": dict(spec=R.Spec(17, 16, 7, 8, ("relu", "relu")), T=40, B=32),
    "bf16-h64": dict(spec=R.Spec(17, 64, 7, 8, ("relu", "relu")), T=3, B=32, precision="bf16"),
    "host-rounds-h64": dict(spec=R.Spec(17, 64, 7, 8, ("relu", "relu")), T=4, B=32, force=1),
    "c2-h256": dict(spec=R.Spec(17, 256, 7, 8, ("relu", "relu")), T=8, B=32),
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_merged_backward_is_bit_exact(case, monkeypatch):
    c = dict(CASES[case])
    spec, T, B = c.pop("spec"), c.pop("T"), c.pop("B")
    on = run_loop(monkeypatch, "1", spec, T, B, 30, **c)
    off = run_loop(monkeypatch, "0", spec, T, B, 30, **c)
    assert_identical(on, off)
    if "force" in c:
        assert on["stats"]["host_round_steps"] > 0, on["stats"]


@pytest.mark.parametrize("spec,T,B,max_batch,n",
                         [(R.Spec(17, 64, 7, 8, ("relu", "relu")), 3, 48, 64, 10),
                          (R.Spec(17, 512, 7, 8, ("relu", "relu")), 2, 8, 8, 6)],
                         ids=["two-row-tiles-b48", "split-n-dx-h512"])
def test_fallback_keeps_the_separate_launch(spec, T, B, max_batch, n, monkeypatch):
    """M > 32 (two 32-row dX tiles per head) and a layer wider than the split-N threshold: NL
    backward launches per round with the switch on as with it off, identical results, and the
    oracle's."""
    n_on, NL = bwd_launches(monkeypatch, "1", spec, T, B, max_batch)
    n_off, _ = bwd_launches(monkeypatch, "0", spec, T, B, max_batch)
    assert n_on == n_off and n_on > 0 and n_on % NL == 0, (n_on, n_off)
    on = run_loop(monkeypatch, "1", spec, T, B, n, max_batch=max_batch, record_oracle=True)
    off = run_loop(monkeypatch, "0", spec, T, B, n, max_batch=max_batch)
    assert_identical(on, off)


def test_merged_round_has_one_backward_launch_fewer(monkeypatch):
    """One update_all of the 4-Linear net: NL - 1 backward launches per round merged, NL unmerged."""
    spec = R.Spec(17, 256, 7, 8, ("relu", "relu"))
    n_on, NL = bwd_launches(monkeypatch, "1", spec, 8, 32)
    n_off, _ = bwd_launches(monkeypatch, "0", spec, 8, 32)
    assert NL == 4
    rounds = n_off // NL
    assert rounds >= 1 and n_off == rounds * NL and n_on == rounds * (NL - 1), (n_on, n_off)
