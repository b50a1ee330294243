"""Timing of df_flow_logpdf_grid beside df_flow_logpdf on the same points.

    python tools/grid_bench.py [--len 16] [--calls 50] [--rounds 6] [--out FILE]

The config-2 chain (bench.py's headline model, d = 5, n = 0) on the len⁵-point grid whose
axes are quantiles of x = forward(z): the grid call (generator kernel + fused logpdf per
chunk, default chunk) against the fused logpdf alone on the points already materialised on
the device.  One process, the two calls alternating round by round, device events around
`calls` launches each, after a warm-up and 0.3 s of untimed rounds.  The two outputs must be
bitwise equal.  Then one clock run of each with the in-kernel stamps on
(df_chain_clock_probe): cycles per launch = ms per call × median shader clock.  Prints one
JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--len", type=int, default=16, dest="length")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--settle-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()

    import torch

    import bench
    import densityflows_amd as dfa
    from densityflows_amd.hip import _ptr, _stream

    if not torch.cuda.is_available():
        raise SystemExit("grid_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    d, n, _ = bench.CONFIGS["cfg2"]
    chain = bench.build_chain("cfg2")
    flow = dfa.Flow(chain, metadata=dfa.MetaData("", d, n, np.zeros(n, np.float32), np.ones(n, np.float32)))
    h = flow.hip(device=0)
    L = args.length
    P = L ** d

    # axes where the flow puts its data: quantiles 0.1 … 0.9 of x = forward(z), per dimension
    gen = torch.Generator(device=dev).manual_seed(7)
    z = torch.randn(d * (1 << 16), device=dev, generator=gen)
    x, ldj = torch.empty_like(z), torch.empty(1 << 16, device=dev)
    h.run("forward", z, None, x, ldj, 1 << 16)
    q = torch.linspace(0.1, 0.9, L, device=dev)
    axes = torch.stack([torch.quantile(x.view(-1, d)[:, k], q) for k in range(d)]).contiguous()   # (d, L)
    axes_buf = axes.reshape(-1)
    lens = (C.c_int64 * d)(*([L] * d))
    # the same points materialised: point p has index (p // L^k) % L on axis k
    p = torch.arange(P, device=dev)
    pts = torch.stack([axes[k][(p // L ** k) % L] for k in range(d)], dim=1).contiguous().reshape(-1)   # (d, P) Julia
    lp_grid = torch.empty(P, device=dev)
    lp_mat = torch.empty(P, device=dev)
    st = _stream(dev)

    def check(rc):
        if rc != 0:
            raise RuntimeError(h.lib.df_last_error().decode())

    grid_args = (h.handle, _ptr(axes_buf), lens, C.c_int64(0), C.c_int64(P), _ptr(lp_grid), C.c_int64(0), st)
    mat_args = (h.handle, _ptr(pts), None, _ptr(lp_mat), C.c_int64(P), st)
    calls = {"grid": lambda: check(h.lib.df_flow_logpdf_grid(*grid_args)),
             "materialised": lambda: check(h.lib.df_flow_logpdf(*mat_args))}

    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    same = bool(torch.equal(lp_grid.view(torch.int32), lp_mat.view(torch.int32)))
    finite = bool(torch.isfinite(lp_mat).all())
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < args.settle_seconds:
        for f in calls.values():
            f()
        torch.cuda.synchronize()

    def timed(f, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    ms = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, f in calls.items():
            ms[name].append(timed(f, args.calls))
    clock = {}
    for name, f in calls.items():
        h.clock_probe(True)
        t = timed(f, args.calls)
        ghz, _, slots = h.clock_read()
        h.clock_probe(False)
        clock[name] = {"clock_run_ms_per_call": round(t, 4), "ghz_median": round(ghz, 4), "workgroup_slots": slots,
                       "mcycles_per_call": round(t * ghz, 4)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    line = {"config": "cfg2", "d": d, "n": n, "axis_length": L, "points": P, "calls_per_round": args.calls,
            "bitwise_equal": same, "finite": finite,
            "ms_per_call": {name: [round(t, 4) for t in v] for name, v in ms.items()},
            "median_ms": {name: round(t, 4) for name, t in med.items()},
            "msamples_per_s": {name: round(P / t / 1e3, 1) for name, t in med.items()},
            "grid_over_materialised": round(med["grid"] / med["materialised"], 4),
            "clock": clock}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    if not (same and finite):
        raise SystemExit("grid and materialised logpdf differ")


if __name__ == "__main__":
    main()
