"""bench.py's plain run (the headline alone) and `--dump-outputs`: the line carries the headline fields and none of `--full`'s,
`--steps` is the number of timed steps, and the files hold what the timed step returned — checked against the same inputs
regenerated here.  Needs an MI355X: `pytest -m gpu`."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_its_dumped_outputs(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 7 and j["warmup"] == 3 and j["n_gpus"] == 1
    assert j["unit"] == "GB/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["ms_per_step"] > 0
    assert abs(j["value"] - j["config"]["algorithmic_bytes_per_step_per_gpu"] / (j["ms_per_step"] * 1e-3) / 1e9) < 0.01 * j["value"]
    for key in ("roofline", "kernels_ms", "c5", "patterns", "published_shapes", "cpu_baseline", "ms_per_step_loops"):
        assert key not in j, key

    files = {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert sorted(files) == ["C.npy", "gradA_col_indices.npy", "gradA_crow_indices.npy", "gradA_values.npy", "gradB.npy"]
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())

    # the same inputs as bench.py's C2 headline (seeded on the device), and the same sample of rows / stored entries
    from torchsparsegradutils_amd.utils import synthetic

    n, p, dev = 100 ** 3, 32, torch.device("cuda:0")
    crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    val = torch.randn(col.numel(), device=dev, generator=g)
    B = torch.randn(n, p, device=dev, generator=g)
    G = torch.randn(n, p, device=dev, generator=g)
    rng = np.random.default_rng(0)
    rows = np.sort(rng.choice(n, size=(1 << 21) // p, replace=False))
    ents = np.sort(rng.choice(col.numel(), size=1 << 19, replace=False))
    crow, col, val, B, G = (t.cpu().double() if t.is_floating_point() else t.cpu().long() for t in (crow, col, val, B, G))
    assert np.array_equal(files["gradA_crow_indices.npy"], crow[rows].numpy())
    assert np.array_equal(files["gradA_col_indices.npy"], col[ents].numpy())
    # C = A·B on the sampled rows, gradA = <G[row], B[col]> on the sampled entries (fp64 here, fp32 in the kernels)
    r = torch.from_numpy(rows)
    starts, counts = crow[r], crow[r + 1] - crow[r]
    slot = torch.repeat_interleave(torch.arange(len(rows)), counts)
    e = torch.repeat_interleave(starts - torch.cumsum(counts, 0) + counts, counts) + torch.arange(int(counts.sum()))
    C = torch.zeros(len(rows), p, dtype=torch.float64).index_add_(0, slot, val[e, None] * B[col[e]])
    assert np.abs(files["C.npy"] - C.numpy()).max() <= 1e-5 * np.abs(C.numpy()).max()
    e = torch.from_numpy(ents)
    row_of = torch.searchsorted(crow, e, right=True) - 1
    gA = (G[row_of] * B[col[e]]).sum(1)
    assert np.abs(files["gradA_values.npy"] - gA.numpy()).max() <= 1e-5 * np.abs(gA.numpy()).max()
    # gradB = Aᵀ·G on the sampled rows: the stored entries whose column is a sampled row
    slot_of = torch.full((n,), -1, dtype=torch.long)
    slot_of[r] = torch.arange(len(rows))
    m = slot_of[col] >= 0
    row_all = torch.repeat_interleave(torch.arange(n), crow[1:] - crow[:-1])
    gB = torch.zeros(len(rows), p, dtype=torch.float64).index_add_(0, slot_of[col[m]], val[m, None] * G[row_all[m]])
    assert np.abs(files["gradB.npy"] - gB.numpy()).max() <= 1e-5 * np.abs(gB.numpy()).max()
