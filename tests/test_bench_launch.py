"""bench.py --gpus N as its own launcher (VERDICT r3 missing #1): the parent starts N rank
processes with the torch.distributed env contract before anything touches a GPU.  Dry-run mode
(SFX_BENCH_DRYRUN=1): each rank prints its env and exits, so this runs on the CPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = dict(os.environ, SFX_BENCH_DRYRUN="1")
    e.pop("WORLD_SIZE", None)
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=300)


def test_gpus_n_starts_n_ranks_with_the_rank_env():
    res = _run(["--gpus", "4", "--steps", "7", "--warmup", "2"])
    assert res.returncode == 0, res.stderr
    lines = [json.loads(x) for x in res.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 4
    assert sorted(int(x["RANK"]) for x in lines) == [0, 1, 2, 3]
    assert all(x["LOCAL_RANK"] == x["RANK"] for x in lines)
    assert {x["WORLD_SIZE"] for x in lines} == {"4"}
    assert {x["MASTER_ADDR"] for x in lines} == {"127.0.0.1"}
    assert len({x["MASTER_PORT"] for x in lines}) == 1
    assert {x["gpus"] for x in lines} == {4}


def test_one_gpu_runs_in_process():
    res = _run(["--gpus", "1"])
    assert res.returncode == 0, res.stderr
    lines = [json.loads(x) for x in res.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1 and lines[0]["RANK"] is None and lines[0]["gpus"] == 1


def test_full_and_dump_outputs_are_options(tmp_path):
    # the dry run parses the whole command line; it touches no GPU and writes nothing
    res = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", str(tmp_path / "out")])
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.splitlines()[-1])["gpus"] == 1 and not (tmp_path / "out").exists()


def test_torchrun_world_must_match_gpus():
    # under an outside launcher (WORLD_SIZE set) the flag is checked, not re-launched
    res = _run(["--gpus", "3"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert res.returncode != 0
    assert "WORLD_SIZE=2" in res.stderr
    ok = _run(["--gpus", "2"], WORLD_SIZE="2", RANK="1", LOCAL_RANK="1")
    assert ok.returncode == 0 and json.loads(ok.stdout.splitlines()[-1])["RANK"] == "1"


def test_a_failing_rank_fails_the_launch():
    # bad arguments end the launch with a nonzero status (nothing hangs waiting for ranks)
    res = _run(["--gpus", "2", "--steps", "notanint"])
    assert res.returncode != 0
