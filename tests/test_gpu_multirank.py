"""8-GPU readiness that one GPU can prove (round 2's review, item 7): bench.py's multi-rank path -- rendezvous on 127.0.0.1,
rank -> device map, contiguous shards of ONE batch ("strong" scaling), every rank's parity sample, the world-size-N gloo MAX
of the timings, one JSON line from rank 0 -- run with all ranks mapped onto device 0.  Three launch shapes: bench.py starting
its own ranks (4 of them), the driver's `python -m torch.distributed.run ... bench.py --gpus N`, and ranks that each see one
visible device (HIP_VISIBLE_DEVICES).  Reference analogue: one job, however many workers (perftest/src/main.rs:39-52).
At most MAX_RANKS ranks share the device: with this test process they are the processes that hold the GPU open at once, and a
shared GPU machine allows no more than six."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
MAX_RANKS = 4


def _one_json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def _check(d, world, total):
    assert d["n_gpus"] == world and d["scaling"] == "strong" and d["value"] and d["value"] > 0
    assert d["config"]["total_frames"] == total and abs(d["config"]["frames_per_gpu"] - total / world) <= 1
    assert d["parity"]["mismatches"] == 0 and d["parity"]["frames_compared"] == 32 * world
    assert d["metric"].startswith("decoded codewords/sec @25 min-sum iters, TM8192")
    assert d["cpu_baseline"] is None and "configs" not in d
    # the line verifies itself: the whole job's exact results against the committed one-GPU answers of bench.EXPECTED_JOBS
    assert d["parity"]["whole_job"]["match"] is True, d["parity"]["whole_job"]
    # ... and explains a slow rank by itself: device, kernel time and the clock held under load, per rank
    assert [r["rank"] for r in d["ranks"]] == list(range(world)) and sum(r["frames"] for r in d["ranks"]) == total
    assert all(r["kernel_ms"] > 0 and r["wall_s"] > 0 and r["device"] == 0 for r in d["ranks"])
    assert all(1000 < r["shader_clock_mhz_under_valu_load"] < 3000 for r in d["ranks"]), d["ranks"]


def test_four_ranks_on_one_gpu_started_by_bench_py():
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(MAX_RANKS), "--devices", ",".join(["0"] * MAX_RANKS), "--total-frames", "65536",
                        "--steps", "2", "--warmup", "1", "--rank-parity-frames", "32", "--no-configs", "--full"], capture_output=True, text=True, cwd=ROOT,
                       timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(_one_json_line(r.stdout), MAX_RANKS, 65536)


def test_two_ranks_under_the_drivers_launcher():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), BENCH, "--gpus", "2", "--devices", "0,0", "--total-frames", "32769", "--steps", "2",
                        "--warmup", "1", "--rank-parity-frames", "32", "--no-configs", "--full"], capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(_one_json_line(r.stdout), 2, 32769)            # an odd total: the shards differ by one frame


def test_ranks_that_each_see_one_visible_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--total-frames", "16384", "--steps", "1", "--warmup", "1",
                        "--rank-parity-frames", "32", "--no-configs", "--full"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(_one_json_line(r.stdout), 2, 16384)


def test_an_n_gpu_job_is_the_one_gpu_job_bit_for_bit():
    """Round 3's review, weak #7 (i): rank r used to generate its shard from its own seed, so an 8-GPU run decoded different bits
    from the one-GPU batch.  Frames are now keyed by their global index, so the job's exact integer results -- sum of the
    iteration counts, failed frames, and the position-weighted digest of every hard decision -- must be EQUAL for 1, 2, 3 and 4
    ranks (all on device 0 here; on the driver's node the same three numbers tie SCALE N=8 to BENCH N=1)."""
    total, seen = 40961, {}
    for world in (1, 2, 3, MAX_RANKS):
        r = subprocess.run([sys.executable, BENCH, "--gpus", str(world), "--devices", ",".join(["0"] * world), "--total-frames", str(total),
                            "--steps", "1", "--warmup", "0", "--no-cpu", "--no-configs", "--full"], capture_output=True, text=True, cwd=ROOT, timeout=1500)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        d = _one_json_line(r.stdout)
        assert d["n_gpus"] == world and d["config"]["total_frames"] == total
        seen[world] = (d["diag"]["job_digest"], d["diag"]["iters_sum"], d["diag"]["failed_frames"], d["diag"]["mean_iters_returned"])
        assert d["parity"]["whole_job"]["match"] is True, d["parity"]["whole_job"]           # against the COMMITTED constants, not only each other
    assert len(set(seen.values())) == 1, seen
    assert seen[1][1] > total * 5 and 0 <= seen[1][2] < total // 10


@pytest.mark.parametrize("dtype,code,ebn0", [("i8", "TM8192", 2.0), ("i8", "TM5120", 4.0)])
def test_the_i8_jobs_verify_themselves_too(dtype, code, ebn0):
    """The bit-sliced i8 kernels behind the same self-check: 1 and 3 ranks reproduce the committed answers of the 40 961-frame jobs."""
    for world in (1, 3):
        r = subprocess.run([sys.executable, BENCH, "--gpus", str(world), "--devices", ",".join(["0"] * world), "--code", code, "--dtype", dtype,
                            "--ebn0", str(ebn0), "--total-frames", "40961", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-configs", "--full"],
                           capture_output=True, text=True, cwd=ROOT, timeout=1500)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        d = _one_json_line(r.stdout)
        assert d["parity"]["whole_job"]["match"] is True, d["parity"]["whole_job"]


@pytest.mark.parametrize("world,frame", [(1, 30000), (3, 30000), (MAX_RANKS, 40960)])
def test_a_corrupted_shard_voids_the_line(world, frame):
    """One flipped output bit in ONE frame of one rank's shard (bench.py --corrupt-frame, a test hook), outside every rank's oracle
    sample: the whole-job digest no longer equals the committed one, the line says so, carries no value, and bench exits non-zero."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(world), "--devices", ",".join(["0"] * world), "--total-frames", "40961", "--steps", "1",
                        "--warmup", "0", "--rank-parity-frames", "32", "--no-configs", "--full", "--corrupt-frame", str(frame)],
                       capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode != 0, r.stdout[-2000:]
    d = _one_json_line(r.stdout)
    assert d["value"] is None and "whole-job" in d["error"]
    w = d["parity"]["whole_job"]
    assert w["match"] is False and w["got"]["job_digest"] != w["expected"]["job_digest"]
    assert w["got"]["iters_sum"] == w["expected"]["iters_sum"] and d["parity"]["mismatches"] == 0      # only the digest sees it


def test_dump_outputs_hold_the_job_the_line_verified(tmp_path):
    """bench.py --dump-outputs: a job small enough to dump whole gives back, from the files alone, the line's own iters_sum,
    failed_frames and job_digest (bench.Workload.sums); a job dumped as a sample holds the same frames from one rank and from three."""
    import numpy as np
    DIGEST_MOD = (1 << 53) - 111

    def run(world, total, outdir):
        r = subprocess.run([sys.executable, BENCH, "--gpus", str(world), "--devices", ",".join(["0"] * world), "--total-frames", str(total),
                            "--steps", "2", "--warmup", "0", "--no-cpu", "--no-configs", "--full", "--dump-outputs", str(outdir)],
                           capture_output=True, text=True, cwd=ROOT, timeout=1500)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        files = {n: np.load(outdir / f"{n}.npy") for n in ("output", "iters", "success")}
        assert all(a.dtype == np.float32 for a in files.values()) and sum(a.nbytes for a in files.values()) < 64 * 10 ** 6
        return _one_json_line(r.stdout), files

    d, f = run(1, 8192, tmp_path / "whole")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    out, iters, succ = f["output"].astype(np.int64), f["iters"].astype(np.int64), f["success"].astype(np.int64)
    assert out.shape == (8192, 1280) and iters.shape == succ.shape == (8192,)
    assert int(iters.sum()) == d["diag"]["iters_sum"] and int((succ == 0).sum()) == d["diag"]["failed_frames"]
    idx = np.arange(8192, dtype=np.int64)
    w = (idx * 0x9E3779B1 + 12345) % 1000003 + 1
    rows = (out * (np.arange(1280) % 251 + 1)).sum(axis=1) + iters * 65537 + succ * 257
    assert f"{int(((rows % 1000003) * w).sum()) % DIGEST_MOD:014x}" == d["diag"]["job_digest"]

    _, one = run(1, 40961, tmp_path / "one")
    _, three = run(3, 40961, tmp_path / "three")
    assert one["output"].shape[0] < 40961
    assert all((one[n] == three[n]).all() for n in one)


def test_a_plain_run_prints_the_headline_alone(tmp_path):
    """Without --full a run sets up, warms up, times its steps, dumps and prints: the line holds the contract's fields and the
    configuration, nothing that takes work of its own.  Its dumped outputs are those of a --full run of the same job, on one
    rank and on two."""
    import numpy as np
    plain_keys = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config"}

    def run(world, outdir, *extra):
        r = subprocess.run([sys.executable, BENCH, "--gpus", str(world), "--devices", ",".join(["0"] * world), "--total-frames", "16384",
                            "--steps", "2", "--warmup", "1", "--dump-outputs", str(outdir), *extra], capture_output=True, text=True, cwd=ROOT,
                           timeout=1500)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        return _one_json_line(r.stdout), {n: np.load(outdir / f"{n}.npy") for n in ("output", "iters", "success")}

    full, want = run(1, tmp_path / "full", "--full", "--no-cpu", "--no-configs")
    assert full["parity"]["whole_job"]["match"] is True, full["parity"]["whole_job"]
    for world in (1, 2):
        d, got = run(world, tmp_path / f"plain{world}")
        assert set(d) == plain_keys, sorted(d)
        assert d["n_gpus"] == world and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["unit"] == "codewords/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["metric"] == full["metric"] and d["config"]["total_frames"] == 16384
        assert d["config"] == full["config"] if world == 1 else d["config"]["library_build"] == full["config"]["library_build"]
        assert all((got[n] == want[n]).all() for n in want)
