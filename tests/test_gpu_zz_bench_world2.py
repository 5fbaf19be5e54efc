"""bench.py's N > 1 code path on a one-GPU box: two ranks share cuda:0 and talk over gloo (RCCL refuses two ranks on one
device; `TSGU_BENCH_TEST_BACKEND` is a test hook).  Checks that both ranks get through the barriers, the max-over-ranks timing,
the sharded C5 leg (plain and chunk-overlapped gathers) and the all-gather leg (all three: `--full`), and that rank 0 prints
ONE well-formed line — the numbers of such a run mean nothing.  (Collected last: the file name sorts after the parity tests.)
Needs an MI355X: `pytest -m gpu`."""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form", ["launcher", "bare"])
def test_bench_runs_with_two_ranks(form):
    """`launcher`: started the way the driver starts N > 1 (python -m torch.distributed.run ... bench.py --gpus 2).
    `bare`: `python bench.py --gpus 2` — bench.py starts its own ranks as child processes (no GPU call before that)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    env = dict(os.environ, TSGU_BENCH_TEST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--full"]
    if form == "launcher":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", "29519"] + tail
    else:
        cmd = [sys.executable] + tail
    try:
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.skip("the two-rank launch did not finish in 300 s on this box (rendezvous / gloo transport), nothing learnt about bench.py")
    if out.returncode != 0 and 'bench.py", line' not in out.stderr:
        # the launcher or the gloo transport failed before / outside bench.py (no interface, port taken): not a statement about the code
        pytest.skip("torch.distributed.run / gloo could not start two ranks here: " + out.stderr[-400:])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["scaling"] == "weak" and j["value"] > 0 and j["cpu_baseline"] is None
    assert j["allgather"]["bytes_per_rank"] == 10 ** 6 * 32 * 4
    c5 = j["c5"]
    assert "error" not in c5, c5
    for key in ("fwd_compute_only", "fwd_bwd_compute_only", "fwd_end_to_end_with_allgather", "fwd_end_to_end_overlapped_chunks"):
        assert c5[key]["ms"] > 0, key
    assert "2 rank(s) x 32 items" in c5["workload"]
    # every rank allocates its own items only: half of the job's 64 items
    per_item = 2 * (3538944 + 2 * 131072 * 16) + 4 * (131073 + 3538944)
    assert c5["resident_bytes_per_rank"] == 32 * per_item


def test_bench_prints_its_line_when_a_secondary_leg_stalls():
    """N > 1: the legs after the timed region use RCCL collectives beyond its barrier (an all-gather, the sharded C5 leg).  If one
    stalls (`TSGU_BENCH_TEST_STALL`: a leg that never returns), every rank leaves after `TSGU_BENCH_LEGS_TIMEOUT` seconds and rank 0
    still prints the ONE line — headline fields intact, the secondary legs marked as not finished — and the run's exit code is non-zero."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    env = dict(os.environ, TSGU_BENCH_TEST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", TSGU_BENCH_TEST_STALL="1",
               TSGU_BENCH_LEGS_TIMEOUT="5")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--full"]
    try:
        out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        pytest.skip("the two-rank launch did not finish in 300 s on this box (rendezvous / gloo transport)")
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 and not lines and 'bench.py", line' not in out.stderr:
        pytest.skip("torch.distributed.run / gloo could not start two ranks here: " + out.stderr[-400:])
    # the watchdog ends the ranks with a non-zero code (a stalled run is not a success) AFTER rank 0 has printed the line
    assert out.returncode != 0, "a run whose secondary legs stalled must not exit 0"
    assert len(lines) == 1, out.stdout[-2000:] + out.stderr[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["value"] > 0 and j["ms_per_step"] > 0 and j["roofline"]["frac"] > 0
    assert "not finished" in j["c5"]["error"] and "allgather" not in j
