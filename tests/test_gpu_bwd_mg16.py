"""The merged last backward launch at 16-column layer-0 tiles (k_bwd_mg): a layer-0
tile of the merged launch is 16 columns wide -- one dX sub-tile, one 16-wide k group of dW per
wave, all four waves sharing the row tiles of the fused forward -- where every other backward
launch keeps the 32-column tile.

Same contract as test_gpu_bwd_merge.py: everything a run leaves behind is IDENTICAL to
SFX_BWD_MERGE=0 (torch.equal on heads, targets, moments, step counts and every action).  The shapes
are the smallest at which a 16-column tile can go wrong and a 32-column one could not: an odd
number of tiles, a last tile 8 columns wide, K > 32 (every wave's k group live), K = KFUSE, K < 16,
the loss tail in the merged launch, bf16 operands, host rounds, five heads per XCD -- and the tiles
of a policy that skips the round (role_v0_only), which share the tile index space.
"""
import pytest

from oracle import ref_cpu as R
from tests.conftest import gpu_available
from tests.test_gpu_bwd_merge import assert_identical, bwd_launches, run_loop

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no HIP device")


RR = ("relu", "relu")
CASES = {
    # three 16-column tiles: code that still thinks in pairs
    "odd-tiles-h48": dict(spec=R.Spec(17, 48, 7, 8, RR), T=3, B=32),
    # last tile 8 columns wide; 7 rows; dZ_1 rows by dword loads
    "ragged-h24-b7": dict(spec=R.Spec(17, 24, 7, 8, RR), T=3, B=7),
    # tiles 16 + 16 + 8
    "ragged-h40": dict(spec=R.Spec(17, 40, 7, 8, RR), T=3, B=32),
    # K > 32: three k groups live; LDS row stride
    "k40": dict(spec=R.Spec(40, 32, 7, 8, RR), T=3, B=32),
    # K = KFUSE, the largest fused fan-in: every wave's k group
    "k64-bound": dict(spec=R.Spec(64, 32, 7, 8, RR), T=2, B=32),
    # one tile, K < 16
    "k4-h16": dict(spec=R.Spec(4, 16, 7, 8, RR), T=3, B=32),
    # the merged launch carries the loss tail
    "one-hidden-h48": dict(spec=R.Spec(17, 48, 7, 8, ("relu",)), T=3, B=32),
    "bf16-h48": dict(spec=R.Spec(17, 48, 7, 8, RR), T=3, B=32, precision="bf16"),
    "host-rounds-h48": dict(spec=R.Spec(17, 48, 7, 8, RR), T=4, B=32, force=1),
    # T A > 256, 5 heads per XCD in xcd_decode
    "t40-h16": dict(spec=R.Spec(17, 16, 7, 8, RR), T=40, B=32),
}
# cases whose run must skip policies (their layer-0 tiles then ran role_v0_only at the new width);
# a property of the training run, so it is asserted on both arms
SKIPS = ("odd-tiles-h48", "ragged-h24-b7")


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_mg16_is_bit_exact(case, monkeypatch):
    c = dict(CASES[case])
    spec, T, B = c.pop("spec"), c.pop("T"), c.pop("B")
    on = run_loop(monkeypatch, "1", spec, T, B, 30, **c)
    off = run_loop(monkeypatch, "0", spec, T, B, 30, **c)
    print(case, "skips on/off", on["skips"], off["skips"], on["stats"])
    assert_identical(on, off)
    if "force" in c:
        assert on["stats"]["host_round_steps"] > 0, on["stats"]
    if case in SKIPS:
        assert off["skips"]["policies_skipped"] > 0, off["skips"]
        assert on["skips"]["policies_skipped"] > 0, on["skips"]


def test_mg16_ragged_tile_matches_oracle(monkeypatch):
    """ragged-h24-b7 once more against oracle/ref_cpu.py, not only against the other arm."""
    c = CASES["ragged-h24-b7"]
    on = run_loop(monkeypatch, "1", c["spec"], c["T"], c["B"], 30, record_oracle=True)
    off = run_loop(monkeypatch, "0", c["spec"], c["T"], c["B"], 30)
    assert_identical(on, off)


def test_mg16_round_has_one_backward_launch_fewer(monkeypatch):
    """Three 16-column tiles per head: NL - 1 backward launches per round merged, NL unmerged."""
    spec = R.Spec(17, 48, 7, 8, RR)
    n_on, NL = bwd_launches(monkeypatch, "1", spec, 3, 32)
    n_off, _ = bwd_launches(monkeypatch, "0", spec, 3, 32)
    assert NL == 4
    rounds = n_off // NL
    assert rounds >= 1 and n_off == rounds * NL and n_on == rounds * (NL - 1), (n_on, n_off)
