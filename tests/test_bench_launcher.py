"""bench.py's multi-rank launch paths, rehearsed on CPU (GAT_BENCH_DRYRUN=1: gloo rendezvous, barrier,
all_gather, one JSON line from rank 0 -- no GPU call).  The driver starts N > 1 through
torch.distributed.run; a plain `python bench.py --gpus N` must start its own N child processes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = dict(os.environ, GAT_BENCH_DRYRUN="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


FAKE_CHECK = (f"{sys.executable} -c \"print('members 2 ...'); "
              "print('{\\\"devices\\\": 2, \\\"members\\\": 2, \\\"bit_identical\\\": true, \\\"peer_copy_GBps\\\": 48.5}')\"")


def _one_line(stdout: str) -> dict:
    lines = [ln for ln in stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_self_launch_two_ranks():
    """The parent (which never touches the GPU) takes rank 0's line, runs the device-group self-check in a further child
    process AFTER every rank has exited, and prints ONE line carrying it."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=dict(_env(), GAT_BENCH_GROUP_CHECK_CMD=FAKE_CHECK), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = _one_line(p.stdout)
    assert rec["n_gpus"] == 2 and rec["ranks_seen"] == [0, 1]
    gc = rec["group_check"]
    assert gc["devices"] == 2 and gc["bit_identical"] is True and gc["peer_copy_GBps"] == 48.5 and gc["rc"] == 0


def test_external_launcher_two_ranks():
    """The driver's form: rank 0 runs the self-check itself (fresh child process) once the process group is gone."""
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29653", BENCH, "--gpus", "2", "--steps", "2",
                        "--warmup", "1"], env=dict(_env(), GAT_BENCH_GROUP_CHECK_CMD=FAKE_CHECK), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = _one_line(p.stdout)
    assert rec["n_gpus"] == 2 and rec["ranks_seen"] == [0, 1]
    assert rec["group_check"]["members"] == 2 and rec["group_check"]["bit_identical"] is True


def test_group_check_failure_is_recorded_not_fatal():
    """A self-check that cannot run (no binary, no JSON) leaves an error record in the line; the measurement stands."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=dict(_env(), GAT_BENCH_GROUP_CHECK_CMD="/nonexistent/gat_multi_gpu"), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "error" in _one_line(p.stdout)["group_check"]
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-group-check"],
                       env=dict(_env(), GAT_BENCH_GROUP_CHECK_CMD=FAKE_CHECK), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "group_check" not in _one_line(p.stdout)


@pytest.mark.parametrize("n, want", [(2, [16, 16]), (3, [11, 11, 10])])
def test_strong_scaling_plan_of_the_constellation_leg(n, want):
    """`constellation_config3`: BASELINE configs[3]'s 32 PRNs cut by ShardPlan(32, N, rank) -- every rank computes its own
    slice as measure() does; contiguous, disjoint, complete (32 / 16 / 8 / 4 per GPU at N = 1 / 2 / 4 / 8)."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--steps", "2", "--warmup", "1", "--no-group-check"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    leg = _one_line(p.stdout)["constellation_config3"]
    assert leg["scaling"] == "strong" and leg["prns_total"] == 32 and leg["prns_by_rank"] == want
    firsts = leg["first_prn_by_rank"]
    assert firsts[0] == 0 and all(firsts[r + 1] == firsts[r] + want[r] for r in range(n - 1)) and firsts[-1] + want[-1] == 32
    sys.path.insert(0, ROOT)
    from gpuacceleratedtracking_amd.sharding import ShardPlan
    assert [ShardPlan(32, 8, r).count for r in range(8)] == [4] * 8 and ShardPlan(32, 1, 0).count == 32


def test_constellation_leg_runs_the_headline_protocol():
    src = open(BENCH).read()
    assert "measure(args, g, torch, dist, world, rank, kwc, args.steps, args.warmup, args.settle, False)" in src
    assert 'channels_total=CONSTELLATION_PRNS' in src and '"scaling": "strong"' in src


def test_shard_leg_runs_the_headline_protocol():
    """N > 1: the configs[3] shard is measured with the same settle / warm-up / steps as the headline (a shortened
    protocol reads the device while it leaves idle: 0.70 instead of 0.58 ms per launch)."""
    src = open(BENCH).read()
    assert "measure(args, g, torch, dist, world, rank, kw3, steps3, args.warmup, args.settle, False)" in src
    assert "steps3 = args.steps" in src and "min(args.settle" not in src and "min(args.warmup" not in src


def test_self_launch_ends_soon_when_one_rank_dies():
    """a rank that exits early (missing device, import error) must not leave its siblings in the rendezvous
    until the launch deadline -- the launcher polls all children, terminates the survivors and returns the failure."""
    import time
    env = dict(_env(), GAT_BENCH_DRYRUN_FAIL_RANK="1", GAT_BENCH_LAUNCH_TIMEOUT="600")
    t0 = time.time()
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 3, (p.returncode, p.stderr[-500:])
    assert time.time() - t0 < 120  # not the 600 s deadline


def test_world_size_mismatch_is_an_error():
    env = dict(_env(), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "WORLD_SIZE" in p.stderr


def test_roofline_names_the_winning_term():
    """configs[1] is HBM-bound on paper, configs[2] (L5, 12 PRNs, 5 taps) and configs[4] are flop-bound."""
    sys.path.insert(0, ROOT)
    import bench

    f1 = bench.algorithmic_flops(4096, 20000, 4, 3, 1)
    b1 = 4096 * (8 * 20000 * 4 + 8 * 4 * 3)
    assert b1 / 8e12 > f1 / 157.3e12
    f3 = bench.algorithmic_flops(1024, 50000, 4, 5, 12)
    b3 = 1024 * (8 * 50000 * 4 + 8 * 4 * 5 * 12)
    assert f3 / 157.3e12 > b3 / 8e12
    assert f3 == pytest.approx(8.72e10, rel=0.01)  # the figure VERDICT r01 quotes for configs[2]


class _FakeOp:
    def __init__(self, out):
        self.out = out

    def result(self):
        return self.out


def test_dump_outputs_writes_the_last_step_and_bounds_its_size(tmp_path, monkeypatch):
    """--dump-outputs: the operator's (re, im) outputs as float32 .npy files; beyond the size limit a fixed seeded sample of
    the flat outputs with its indices, the same from run to run."""
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench

    rng = np.random.default_rng(5)
    out = (rng.standard_normal((6, 2, 3, 4)) + 1j * rng.standard_normal((6, 2, 3, 4))).astype(np.complex64)
    rec = bench.dump_outputs(str(tmp_path / "a"), {"op": _FakeOp(out)}, 0, 1)
    assert sorted(rec["files"]) == ["out_im.npy", "out_re.npy"] and not rec["sampled"] and rec["shape"] == [6, 2, 3, 4]
    re, im = np.load(tmp_path / "a" / "out_re.npy"), np.load(tmp_path / "a" / "out_im.npy")
    assert re.dtype == np.float32 and np.array_equal(re + 1j * im, out)
    rec = bench.dump_outputs(str(tmp_path / "r"), {"op": _FakeOp(out)}, 1, 2)
    assert sorted(rec["files"]) == ["out_im_rank1.npy", "out_re_rank1.npy"]

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 * 10)
    for d in ("s1", "s2"):
        rec = bench.dump_outputs(str(tmp_path / d), {"op": _FakeOp(out)}, 0, 1)
        assert rec["sampled"]
    total = sum(os.path.getsize(tmp_path / "s1" / f) for f in rec["files"]) - 3 * 128  # (.npy headers)
    assert total <= 16 * 10
    idx = np.load(tmp_path / "s1" / "sample_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "s2" / "sample_index.npy"))
    flat = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "s1" / "out_re.npy"), out.real.reshape(-1)[flat])
