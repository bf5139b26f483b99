"""Host tests of bench.py's launcher: `python bench.py --gpus N` starts N ranks itself (one process per GPU, the way the
reference's distributed tests start themselves, test/test_distributed_sea_ice.jl:41-54), relays rank 0's JSON line and
never falls back to fewer ranks.  No GPU needed: the plan is printed, the process plumbing runs over gloo."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(*argv, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH, *argv], env=e, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_print_launch_is_one_rank_per_gpu_on_localhost(n):
    p = run("--gpus", str(n), "--steps", "3", "--print-launch")
    assert p.returncode == 0, p.stderr
    plan = json.loads(p.stdout.strip().splitlines()[-1])
    cmd = plan["launch"]
    assert plan["ranks"] == n and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert f"--nproc-per-node={n}" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    tail = cmd[cmd.index(BENCH) + 1:]
    assert tail == ["--gpus", str(n), "--steps", "3"]              # the ranks get the parent's arguments, without --print-launch
    assert plan["would_run"] == (plan["visible_gpus"] >= n)


def test_refuses_to_run_on_fewer_gpus():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs are visible")
    p = run("--gpus", "2", "--steps", "1", "--warmup", "0")
    assert p.returncode == 2 and "refusing to fall back" in p.stderr and p.stdout.strip() == ""


def test_gpus_must_match_world_size():
    p = run("--gpus", "2", env={"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr
    p = run("--gpus", "3")
    assert p.returncode != 0


def test_parent_starts_ranks_and_relays_rank0_line():
    p = run("--gpus", "2", "--self-test-launch")
    assert p.returncode == 0, p.stderr
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1                                         # exactly ONE line on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["self_test"] and out["launched_by_parent"]


def test_plain_run_options():
    """--full is off by default, --steps sets the timed steps, --dump-outputs takes a directory; no timed steps is refused."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs == ""
    a = bench.parse_args(["--full", "--dump-outputs", "some/dir"])
    assert a.full is True and a.dump_outputs == "some/dir"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_fixed_samples_of_large_fields(tmp_path):
    """A 2048^2 tile (the headline grid) is larger than a dump may hold in full: every field is written at the same seeded positions,
    the same on every call, with those positions beside them; 64 MB at most in all.  A small field is written whole."""
    sys.path.insert(0, ROOT)
    import types
    import numpy as np
    import bench

    def fake(n, rank=0):
        rng = np.random.default_rng(5)
        mk = lambda: types.SimpleNamespace(interior_numpy=(lambda a=rng.standard_normal((n, n)): a))
        aux = types.SimpleNamespace(s11=mk(), s22=mk(), s12=mk())
        model = types.SimpleNamespace(synchronize=lambda: None, velocities=types.SimpleNamespace(u=mk(), v=mk()),
                                      dynamics=types.SimpleNamespace(auxiliaries=types.SimpleNamespace(fields=aux)))
        return types.SimpleNamespace(rank=rank, np=np, model=model, tg=types.SimpleNamespace(Nx=n, Ny=n), SIG=bench.Rank.SIG)

    R = fake(2048)
    for d in ("a", "b"):
        bench.dump_outputs(R, str(tmp_path / d))
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["s11.npy", "s12.npy", "s22.npy", "sample_index.npy", "u.npy", "v.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 << 20
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.dtype == np.float64 and idx.size == bench.DUMP_MAX_VALUES and np.all(np.diff(idx) > 0)
    u = R.model.velocities.u.interior_numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "u.npy"), u.reshape(-1)[idx.astype(np.int64)])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    small = fake(64)
    bench.dump_outputs(small, str(tmp_path / "c"))
    assert not (tmp_path / "c" / "sample_index.npy").exists()
    assert np.array_equal(np.load(tmp_path / "c" / "v.npy"), small.model.velocities.v.interior_numpy())
    bench.dump_outputs(fake(64, rank=1), str(tmp_path / "d"))
    assert not (tmp_path / "d").exists()                           # rank 0 alone writes
