"""The N > 1 path end to end on the GPU box: two ranks (gloo; both on the one GPU) run ShardedTriRenderer -- tile-row
bands, gradients written into the flat buffer, ONE all-reduce -- and each compares with the full render."""
import json
import os
import subprocess
import sys

import pytest

from harness import run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, timeout, **env):
    """bench.py with `argv` outside any launcher's environment -> its JSON lines, parsed."""
    clean = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv, "--no-cpu-baseline"], env=dict(clean, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def test_two_ranks_match_full_render(hip_device):
    run_ranks("base", "sharded ok")


def test_bench_gpus_2_rehearsal(hip_device):
    """`python bench.py --gpus 2` with no launcher around it starts two ranks itself: here both
    share the one GPU over gloo; the line must say n_gpus 2 and carry the sharded parallelism."""
    lines = _bench("--gpus", "2", "--config", "C2", "--steps", "3", "--warmup", "1", timeout=600,
                   DMR_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    assert len(lines) == 1, lines
    j = lines[0]
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["value"] > 0
    assert "x2" in j["config"]["parallelism"]
    assert j["sharded_grad_max_norm_err"] is not None and j["sharded_grad_max_norm_err"] <= 5e-5


def test_bench_emulated_view_band(hip_device):
    """C5 has B = 4 views: rank 5 of 8 renders its (view, band) segments (sharding.view_shares) with B = 1 tensors."""
    j = _bench("--config", "C5", "--emulate-rank", "5/8", "--steps", "2", "--warmup", "1", timeout=600)[0]
    assert "segments [(" in j["config"]["parallelism"] and j["value"] > 0


def test_bench_gpus_2_view_segments(hip_device):
    """`bench.py --gpus 2 --config C5`: two ranks (gloo, one GPU) step their (view, band) segments of the four views with
    B = 1 tensors and join ONE all-reduce over the all-views payload."""
    j = _bench("--gpus", "2", "--config", "C5", "--steps", "2", "--warmup", "1", "--settle-ms", "0", timeout=900,
               DMR_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")[0]
    assert j["n_gpus"] == 2 and j["value"] > 0
    assert "segments of 4 views x2" in j["config"]["parallelism"]
    assert j["config"]["allreduce_payload_bytes"] == 80320640
    assert j["sharded_grad_max_norm_err"] is not None and j["sharded_grad_max_norm_err"] <= 5e-5
