"""Cost of sample weights on the training step and the device epoch.

    timeout 900 python tools/weights_bench.py [--repeats 5] [--steps 20] [--other-lib FILE] [--out FILE]

Three workloads, each timed unweighted and weighted, alternating the two paths within one
process after a warm-up of both:
  cfg2_step    config 2 (4 CouplingBlocks, hidden 64), one train step at B = 2^20
  cfg4_step    the config-4/5 model (8 CouplingBlocks, d = 32, n = 8, hidden 256) at B = 2^18,
               the benchmark's batch for it
  readme_epoch the README chain, one HIPTrainer.epoch over 64,000 resident samples at
               batchsize 64 (1000 captured steps)
A step is gradient + update + repack (HIPTrainer.step) on buffers that stay; the weights are
U(0.1, 1.1).  Per workload and path: ms of every repeat (each `--steps` steps or one epoch),
the median, the spread (max − min), and weighted / unweighted of the medians.

--other-lib FILE: a second build of libdensityflows_hip.so (the parent commit's).  The
unweighted paths are then timed in fresh child processes, alternating this build and the other
one `--repeats` times within this one call; the line reports both builds' medians and spreads,
so the difference can be held against the other build's own spread.  (A child process per
measurement: one process binds one library.)
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def _summary(ms):
    return {"ms": [round(v, 4) for v in ms], "median_ms": round(statistics.median(ms), 4),
            "spread_ms": round(max(ms) - min(ms), 4)}


def _step_workload(config, B, steps, repeats, weighted_too):
    import torch

    import bench
    from densityflows_amd.train import Adam, HIPTrainer

    dev = torch.device("cuda", 0)
    d, n, _ = bench.CONFIGS[config]
    chain = bench.build_chain(config)
    hc = chain.hip(device=0, n_hint=n)
    gen = torch.Generator(device=dev).manual_seed(1000)
    z = torch.randn(B * d, device=dev, generator=gen)
    th = torch.rand(B * n, device=dev, generator=gen) if n > 0 else None
    x = torch.empty_like(z)
    hc.run("forward", z, th, x, torch.empty(B, device=dev), B)
    w = torch.rand(B, device=dev, generator=gen) + 0.1
    tr = HIPTrainer(hc, Adam(1e-3))
    paths = {"unweighted": lambda: tr.step(x, th, B)}
    if weighted_too:
        paths["weighted"] = lambda: tr.step(x, th, B, w=w)
    times = {k: [] for k in paths}
    for f in paths.values():      # warm-up: allocations of both paths
        f()
        f()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: _summary(v) for k, v in times.items()}


def _epoch_workload(N, bs, repeats, weighted_too):
    import torch

    import bench
    from densityflows_amd.train import Adam, HIPTrainer

    dev = torch.device("cuda", 0)
    chain = bench.build_chain("cfg1")
    hc = chain.hip(device=0, n_hint=1)
    rng = np.random.default_rng(0)
    xs = torch.from_numpy(rng.standard_normal(N * 5).astype(np.float32)).to(dev)
    ts = torch.from_numpy(rng.random(N).astype(np.float32)).to(dev)
    ws = torch.from_numpy((rng.random(N) + 0.1).astype(np.float32)).to(dev)
    od = torch.from_numpy(rng.permutation(N).astype(np.int32)).to(dev)
    trs = {"unweighted": HIPTrainer(hc, Adam(1e-3))}
    if weighted_too:
        # (a trainer repacks its chain: the weighted one gets its own)
        trs["weighted"] = HIPTrainer(bench.build_chain("cfg1").hip(device=0, n_hint=1), Adam(1e-3))
    run = {"unweighted": lambda t: t.epoch(xs, ts, N, od, bs), "weighted": lambda t: t.epoch(xs, ts, N, od, bs, w=ws)}
    times = {k: [] for k in trs}
    for k, t in trs.items():      # warm-up: the eager first sight and the capture
        run[k](t)
        run[k](t)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, t in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run[k](t)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: _summary(v) for k, v in times.items()}


def measure(args, weighted_too):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("weights_bench needs an MI355X: no HIP device visible")
    res = {"cfg2_step": _step_workload("cfg2", 1 << 20, args.steps, args.repeats, weighted_too),
           "cfg4_step": _step_workload("cfg4", 1 << 18, max(2, args.steps // 4), args.repeats, weighted_too),
           "readme_epoch": _epoch_workload(64000, 64, args.repeats, weighted_too)}
    if weighted_too:
        for v in res.values():
            v["weighted_over_unweighted"] = round(v["weighted"]["median_ms"] / v["unweighted"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="steps per repeat of cfg2_step (a quarter for cfg4_step)")
    ap.add_argument("--other-lib", default=None, help="another build's libdensityflows_hip.so for the A/B")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.child:  # one A/B measurement: the unweighted paths of whatever library the environment names
        print(json.dumps(measure(args, weighted_too=False)))
        return
    res = {"repeats": args.repeats, "steps": args.steps, "this_build": measure(args, weighted_too=True)}
    if args.other_lib:
        libs = {"this": os.path.join(ROOT, "densityflows.jl_amd", "libdensityflows_hip.so"),
                "other": os.path.abspath(args.other_lib)}
        got = {k: [] for k in libs}
        for _ in range(args.repeats):
            for k, path in libs.items():
                env = dict(os.environ, DENSITYFLOWS_HIP_LIB=path)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", "1", "--steps",
                                    str(args.steps)], env=env, capture_output=True, text=True, timeout=300, check=True)
                got[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
        ab = {}
        for wl in ("cfg2_step", "readme_epoch", "cfg4_step"):
            ab[wl] = {k: _summary([g[wl]["unweighted"]["median_ms"] for g in got[k]]) for k in libs}
            ab[wl]["this_minus_other_ms"] = round(ab[wl]["this"]["median_ms"] - ab[wl]["other"]["median_ms"], 4)
        res["unweighted_ab"] = ab
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
