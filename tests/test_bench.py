"""bench.py plumbing on CPU: `--gpus N` self-launching (one rank per GPU through
torch.distributed.run), the loud failure without enough devices, the
roofline pricing of the training step and --dump-outputs; on the GPU, one
plain run and its dump."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(args, env_extra, timeout=240):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", **env_extra)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          env=env, timeout=timeout, cwd=ROOT)


def test_gpus2_self_launches_two_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"], {"DF_DIST_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout           # rank 0 prints ONE line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["dry_run"] is True


def test_gpus2_without_devices_fails_loudly():
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("this host has two GPUs")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"DF_DIST_BACKEND": "nccl"})
    assert r.returncode != 0
    assert "GPU(s) visible" in (r.stderr + r.stdout)
    assert '"n_gpus": 1' not in r.stdout


def test_train_split_flops_pricing():
    import bench

    cfg2 = bench.build_chain("cfg2")
    # 16 nets (in 2/3, hidden 64, out 3/2): forward first + hidden Dense, and the hidden
    # Dense's W1ᵀδ and dW1 on the split products
    hidden = 16 * 2 * 64 * 64
    first = sum(2 * D.in_dim * D.out_dim for e in cfg2 for L in (e.layer_1, e.layer_2)
                for net in (L.s_net, L.t_net) for D in net[:1])
    assert bench.train_split_flops(cfg2, 4) == first + 3 * hidden
    assert bench.train_split_flops(cfg2, 3) == 0.0
    cfg4 = bench.build_chain("cfg4")
    per_net = 2 * (24 * 256 + 256 * 256 + 256 * 16) + 2 * 2 * 256 * 256
    assert bench.train_split_flops(cfg4, 6) == 32 * per_net


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: arrays below the budget are written whole (f32 / f64 kept); above
    it every array is cut to the same fraction at indices fixed by its length."""
    import numpy as np

    import bench

    x = np.arange(5000, dtype=np.float32)
    s = np.array([1.5, 2.0])
    bench.dump_outputs(str(tmp_path / "a"), {"x": x, "s": s})
    xa, sa = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "s.npy")
    assert xa.dtype == np.float32 and sa.dtype == np.float64
    assert np.array_equal(xa, x) and np.array_equal(sa, s)

    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    y = x[::-1].copy()
    bench.dump_outputs(str(tmp_path / "b"), {"x": x, "y": y})
    bench.dump_outputs(str(tmp_path / "c"), {"x": x, "y": y})
    xb, yb = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "b" / "y.npy")
    assert xb.nbytes + yb.nbytes <= 4096 and xb.size == yb.size > 400
    idx = xb.astype(np.int64)                       # x[i] == i: the sample names its indices
    assert np.all(np.diff(idx) > 0) and np.array_equal(yb, y[idx])
    assert np.array_equal(xb, np.load(tmp_path / "c" / "x.npy"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_step(cuda, tmp_path):
    """A plain run prints the headline line without the --full legs and --dump-outputs
    writes x and ldj of the last timed step: the same bits as the forward pass of the
    same model on the same seeded inputs."""
    import numpy as np
    import torch

    import bench

    B, out = 3001, tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B), "--settle-seconds", "0",
              "--dump-outputs", str(out)], {})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "Msamples/s"
    assert line["clock"] is None and "cpu_baseline" not in line and "f32_exact_kernel" not in line
    x, ldj = np.load(out / "x.npy"), np.load(out / "ldj.npy")
    assert x.dtype == np.float32 and x.shape == (5 * B,) and ldj.shape == (B,)

    hc = bench.build_chain("cfg2").hip(device=0, n_hint=0)
    gen = torch.Generator(device=cuda).manual_seed(1000)
    z = torch.randn(B * 5, device=cuda, generator=gen)
    xr, lr = torch.empty_like(z), torch.empty(B, device=cuda)
    hc.run("forward", z, None, xr, lr, B)
    torch.cuda.synchronize()
    assert np.array_equal(x, xr.cpu().numpy()) and np.array_equal(ldj, lr.cpu().numpy())


def test_gpus8_dry_run_reports_every_rank():
    """the 1→8 run is self-diagnosing — 8 ranks launched by
    bench.py itself (gloo on CPU), rank 0 reports n_gpus 8 and the per-rank
    timing spread gathered from all 8."""
    r = _run(["--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run"], {"DF_DIST_BACKEND": "gloo"},
             timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["dry_run"] is True
    ranks = out["ranks"]
    assert ranks["n"] == 8 and ranks["group_size"] == 8 and len(ranks["kernel_ms_per_rank"]) == 8
    assert ranks["wall_ms_per_step_min"] <= ranks["wall_ms_per_step_max"]
    assert ranks["process_group"] == "torch.distributed gloo"
