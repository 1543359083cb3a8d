"""The fused TD launch at 16-row tiles (k_bwd_tdg): where two row tiles per
policy still leave every workgroup a compute unit of its own, a tile of the launch covers 16 rows
of the minibatch instead of 32 -- half the ψ rows of the policy's GPI, one accumulator block -- and
the step counters and Adam constants of the round are computed by a workgroup of their own, past the
tiles, instead of by tile 0 of every head.

Same contract as test_gpu_bwd_mg16.py: everything a run leaves behind is IDENTICAL between
SFX_TDG_ROWS=16 and SFX_TDG_ROWS=32 (torch.equal on heads, targets, moments, step counts, every
action, and the skip statistics).  The shapes are the smallest at which a 16-row tile can go wrong
and a 32-row tile could not: two full tiles, a second tile of one row, of 15 rows; one tile (which
must keep the block vote under either setting); d = 4 / 8 (k_bwd_tdg<2, .>) and d = 16
(k_bwd_tdg<4, .>); A d = 128 (two waves per 64-wide chunk) and A d <= 64; 32 T A = 2048, the bound
of the dots per thread; a last k-tile 8 columns wide and a single k-tile; host rounds; the unfused
TD launch (T = 40), which the switch must not touch; the sharded step's maxima path.

Round skipping: with two row tiles per policy no workgroup sees all of a policy's rows, so the
publishing workgroup of each row tile reports its rows' verdict (tdg_skip_report) where one tile
votes block-wide -- the statistics must count the same on both arms, and the cases in SKIPS must
skip policies.
"""
import pytest
import torch

from oracle import ref_cpu as R
from tests.conftest import gpu_available
from tests.test_gpu_bwd_merge import assert_identical, run_loop

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


RR = ("relu", "relu")
CASES = {
    # two full 16-row tiles; A d = 56: four waves share the one 64-wide chunk
    "b32": dict(spec=R.Spec(17, 48, 7, 8, RR), T=3, B=32),
    # second tile: one row
    "b17": dict(spec=R.Spec(17, 48, 7, 8, RR), T=3, B=17),
    # second tile: 15 rows
    "b31": dict(spec=R.Spec(17, 48, 7, 8, RR), T=3, B=31),
    # one tile: the block vote, whatever the switch says
    "b16": dict(spec=R.Spec(17, 48, 7, 8, RR), T=3, B=16),
    "b7": dict(spec=R.Spec(17, 48, 7, 8, RR), T=3, B=7),
    # d = 4: one float4 per dot
    "d4": dict(spec=R.Spec(17, 48, 7, 4, RR), T=3, B=32),
    # d = 16, T A = 24: k_bwd_tdg<4, 2, 16>; A d = 128: two waves per chunk, 8 k-steps each
    "d16-ad128": dict(spec=R.Spec(17, 48, 8, 16, RR), T=3, B=32),
    # A d = 128 at d = 8
    "d8-ad128": dict(spec=R.Spec(17, 32, 16, 8, RR), T=3, B=31),
    # 32 T A = 2048: every dot slot of the 32-row tile (8 per thread) and of the 16-row tile (4) live
    "ta-bound-t8a8": dict(spec=R.Spec(17, 32, 8, 8, RR), T=8, B=32),
    # hidden width 24: the last k-tile has 8 columns; 16: one k-tile
    "h24": dict(spec=R.Spec(17, 24, 7, 8, RR), T=3, B=32),
    "h16-b17": dict(spec=R.Spec(17, 16, 7, 8, RR), T=3, B=17),
    "host-rounds": dict(spec=R.Spec(17, 48, 7, 8, RR), T=4, B=32, force=1),
    # T A > 256: the TD target is a launch of its own
    "t40-h16": dict(spec=R.Spec(17, 16, 7, 8, RR), T=40, B=32),
    # the headline's shape
    "c2-h256": dict(spec=R.Spec(17, 256, 7, 8, RR), T=8, B=32),
}
# cases whose run must skip policies: on the 16-row arm the per-tile reports decided them
SKIPS = ("b32", "b17", "b31", "h24")


def both_arms(monkeypatch, c, n=30):
    c = dict(c)
    spec, T, B = c.pop("spec"), c.pop("T"), c.pop("B")
    out = []
    for rows in ("16", "32"):
        monkeypatch.setenv("SFX_TDG_ROWS", rows)
        out.append(run_loop(monkeypatch, "1", spec, T, B, n, **c))
    return out


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_tdg_16_row_tiles_are_bit_exact(case, monkeypatch):
    c = CASES[case]
    r16, r32 = both_arms(monkeypatch, c)
    print(case, "skips 16/32", r16["skips"], r32["skips"], r16["stats"])
    assert_identical(r16, r32)
    assert r16["skips"] == r32["skips"], (r16["skips"], r32["skips"])
    if "force" in c:
        assert r16["stats"]["host_round_steps"] > 0, r16["stats"]
    if case in SKIPS:
        assert r32["skips"]["policies_skipped"] > 0, r32["skips"]
        assert r16["skips"]["policies_skipped"] > 0, r16["skips"]


def test_tdg_16_row_tiles_match_oracle(monkeypatch):
    """b17 once more against oracle/ref_cpu.py, not only against the other arm."""
    c = CASES["b17"]
    monkeypatch.setenv("SFX_TDG_ROWS", "16")
    run_loop(monkeypatch, "1", c["spec"], c["T"], c["B"], 30, record_oracle=True)


def test_row_tiles_that_disagree(monkeypatch):
    """Steps in which one row tile of a policy repeats round 0's next actions and the other does
    not: the repeating tile must not skip anything (the policy is not skipped), and the policy must
    count as checked, not as skipped.  Found by reading both rounds' published next actions
    (sfx_debug_spec_next) after every update_all of two device rounds that no host round followed;
    per such step the skip counter must grow by exactly the policies whose two tiles both repeat."""
    from tests.test_gpu_runner import make

    spec, T, B = R.Spec(17, 48, 7, 8, RR), 3, 32
    out = {}
    for rows in ("16", "32"):
        monkeypatch.setenv("SFX_TDG_ROWS", rows)
        eng, _ = make(spec, T, 1000, max_batch=B)
        eng.set_spec_rounds(2)
        gen = torch.Generator().manual_seed(3)
        mixed, nexts = [], []
        for k in range(30):
            s, s1 = torch.randn(B, spec.n_s, generator=gen), torch.randn(B, spec.n_s, generator=gen)
            a = torch.randint(0, spec.A, (B,), generator=gen)
            phi = torch.rand(B, spec.d, generator=gen)
            st0, sk0 = eng.step_stats(), eng.skip_stats()
            eng.update_all(s.cuda(), a.cuda(), phi.cuda(), s1.cuda(), torch.full((B,), 0.9).cuda())
            nx = eng.debug_spec_next(B)
            st1, sk1 = eng.step_stats(), eng.skip_stats()
            nexts.append(nx)
            if st1["host_round_steps"] != st0["host_round_steps"]:
                continue  # host rounds reused the two buffers
            lo = [torch.equal(nx[0, p, :16], nx[1, p, :16]) for p in range(T)]
            hi = [torch.equal(nx[0, p, 16:], nx[1, p, 16:]) for p in range(T)]
            assert sk1["policies_checked"] - sk0["policies_checked"] == T, (k, sk0, sk1)
            assert sk1["policies_skipped"] - sk0["policies_skipped"] == sum(x and y for x, y in zip(lo, hi)), (k, lo, hi)
            mixed += [(k, p) for p in range(T) if lo[p] != hi[p]]
        out[rows] = dict(heads=torch.stack([eng.get_head(t, 0) for t in range(T)]),
                         moms=[eng.get_adam(t) for t in range(T)], mixed=mixed, nexts=torch.stack(nexts),
                         skips=eng.skip_stats())
        eng.close()
    r16, r32 = out["16"], out["32"]
    print("steps with disagreeing row tiles (step, policy):", r16["mixed"], r16["skips"])
    assert len(r16["mixed"]) > 0 and r16["mixed"] == r32["mixed"]
    assert torch.equal(r16["nexts"], r32["nexts"]) and torch.equal(r16["heads"], r32["heads"])
    for (ma, va, sa), (mb, vb, sb) in zip(r16["moms"], r32["moms"]):
        assert torch.equal(ma, mb) and torch.equal(va, vb) and sa == sb
    assert r16["skips"] == r32["skips"] and r16["skips"]["policies_skipped"] > 0


@pytest.mark.parametrize("b", [32, 17])
def test_tdg_16_row_tiles_sharded_step(b, monkeypatch):
    """The sharded all-task step at one rank (tests/test_gpu_shard.py): the TD launch reads the
    all-reduced maxima (tdg_xmax) instead of reducing over heads itself."""
    from tests import test_gpu_shard as S

    cfg = dict(spec=S.SPEC, tg=S.TG, b=b, steps=S.STEPS)
    out = {}
    for rows in ("16", "32"):
        monkeypatch.setenv("SFX_TDG_ROWS", rows)
        out[rows] = S._run_rank(0, 1, 2, lambda t: None, cfg)
    (a16, h16, t16, w16, _), (a32, h32, t32, w32, _) = out["16"], out["32"]
    assert a16 == a32
    assert torch.equal(h16, h32) and torch.equal(t16, t32) and torch.equal(w16, w32)
    want, st = S._oracle(cfg)
    S._check(a16, h16, t16, w16, want, st)


@pytest.mark.parametrize("rows", ["16", "32"])
def test_adam_step_workgroup_commits_nothing_when_cancelled(rows, monkeypatch):
    """The step counters and Adam constants are bumped by a workgroup of their own in the fused TD
    launch.  With a gate bound of 10 ns pre-launched steps are cancelled and re-issued
    (test_gpu_runner.py checks the parameters at B = 16): at B = 32 -- the two-tile shape -- every
    head's step counter must equal the number of updates that committed, no more, and the run must
    still be the oracle's step for step."""
    from sfx.runner import NativeEnvLoop
    from tests.test_gpu_runner import check_state, make, replay_with_oracle

    monkeypatch.setenv("SFX_TDG_ROWS", rows)
    spec = R.Spec(17, 32, 7, 8, RR)
    T, ev, alpha, n, B = 3, 1000, 0.05, 20, 32
    eng, st = make(spec, T, ev, max_batch=B)
    loop = NativeEnvLoop(eng, batch=B, capacity=200, gamma=0.9, epsilon=0.3, alpha_w=alpha, episode_len=7, seed=5)
    loop.prefill(B)
    loop.set_task(1)
    loop.set_gate_timeout(1e-8)
    loop.record(4 * n)
    for _ in range(4):  # a graph's first step races the host: run until some step was cancelled (bounded)
        loop.run(n)
        stats = loop.stats()
        if stats["retried"] > 0:
            break
    assert stats["retried"] > 0, stats
    loop.set_gate_timeout(5.0)
    loop.run(4)  # and normal steps after the cancelled ones
    recs = loop.records()
    updates = sum(1 for r in recs if r["have"])
    assert updates > 0
    assert [eng.get_adam(t)[2] for t in range(T)] == [updates] * T
    replay_with_oracle(st, spec, recs, alpha, ev, loop.action())
    check_state(eng, st, T, len(recs))
    loop.close()
    eng.close()
