"""Timing of df_flow_pdf_marginals beside df_flow_logpdf_grid on the same grid.

    timeout -k 10 300 python tools/time_marginals.py [--calls 20] [--rounds 6] [--out FILE]

Three grids, each with the full corner request (the total, 5 singles, 10 pairs: 16 tables):
the config-2 chain (bench.py's headline model, d = 5) at 16 points per axis (2²⁰ points, one
chunk) and at 32 points per axis (2²⁵ points, 32 chunks), and the README chain (config 1,
one θ value) at 16 points per axis.  Axes are quantiles 0.1 … 0.9 of x = forward(z), weights
the trapezoid rule's.  One process; per grid the two calls alternate round by round, device
events around `calls` launches each, after a warm-up and 0.3 s of untimed rounds.  The
yardstick is df_flow_logpdf_grid, which writes the grid-sized logpdf array the marginal call
does not.  The tables are checked against a float64 reduction of that array with torch.  Then
one clock run of each call with the in-kernel stamps on (df_chain_clock_probe).  Prints one
JSON line per grid.
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--settle-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import bench
    import densityflows_amd as dfa
    from densityflows_amd.hip import _ptr, _stream

    if not torch.cuda.is_available():
        raise SystemExit("time_marginals needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    st = _stream(dev)

    def timed(f, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    ok = True
    for config, L, calls in (("cfg2", 16, args.calls), ("cfg2", 32, max(1, args.calls // 8)), ("cfg1", 16, args.calls)):
        d, n, _ = bench.CONFIGS[config]
        chain = bench.build_chain(config)
        flow = dfa.Flow(chain, metadata=dfa.MetaData("", d, n, np.zeros(n, np.float32), np.ones(n, np.float32)))
        h = flow.hip(device=0)
        if n:
            h.set_theta_bounds(np.zeros(n, np.float32), np.ones(n, np.float32))
        na, P = d + n, L ** d

        # axes where the flow puts its data: quantiles 0.1 … 0.9 of x = forward(z), per dimension
        B = 1 << 16
        gen = torch.Generator(device=dev).manual_seed(7)
        z = torch.randn(d * B, device=dev, generator=gen)
        th = torch.full((n * B,), 0.5, device=dev) if n else None
        x, ldj = torch.empty_like(z), torch.empty(B, device=dev)
        h.run("forward", z, th, x, ldj, B, flow=bool(n))
        q = torch.linspace(0.1, 0.9, L, device=dev)
        xa = [torch.quantile(x.view(-1, d)[:, k], q).contiguous() for k in range(d)]
        parts = xa + [torch.full((1,), 0.5, device=dev) for _ in range(n)]
        axes_buf = torch.cat(parts).contiguous()
        lens_t = [L] * d + [1] * n
        lens = (C.c_int64 * na)(*lens_t)
        w = [dfa.trapezoid_weights(a.cpu().numpy()) for a in parts]
        wbuf = torch.from_numpy(np.concatenate(w)).to(dev)
        keeps = [()] + [(a,) for a in range(d)] + [(a, b) for a in range(d) for b in range(a + 1, d)]
        flat = [v for K in keeps for v in (K + (-1, -1))[:2]]
        req = (C.c_int32 * len(flat))(*flat)
        sizes = [L ** len(K) for K in keeps]
        out = torch.empty(sum(sizes), dtype=torch.float64, device=dev)
        lp = torch.empty(P, device=dev)

        def check(rc):
            if rc != 0:
                raise RuntimeError(h.lib.df_last_error().decode())

        grid_args = (h.handle, _ptr(axes_buf), lens, C.c_int64(0), C.c_int64(P), _ptr(lp), C.c_int64(0), st)
        marg_args = (h.handle, _ptr(axes_buf), _ptr(wbuf), lens, C.c_int64(0), C.c_int64(P), req,
                     C.c_int32(len(keeps)), _ptr(out), C.c_int64(0), st)
        fns = {"grid": lambda: check(h.lib.df_flow_logpdf_grid(*grid_args)),
               "marginals": lambda: check(h.lib.df_flow_pdf_marginals(*marg_args))}

        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        # the tables against a float64 reduction of the grid call's own values
        pdf = torch.exp(lp.double()).reshape([1] * n + [L] * d)         # torch is row-major: axis 0 last
        wt = [torch.from_numpy(v).to(dev) for v in w]
        worst, at = 0.0, 0
        for K, size in zip(keeps, sizes):
            t = pdf
            for k in range(d):
                if k not in K:
                    shape = [1] * na
                    shape[na - 1 - k] = L
                    t = t * wt[k].reshape(shape)
            dims = [na - 1 - k for k in range(na) if k not in K]
            want = t.sum(dim=dims).reshape(-1) if dims else t.reshape(-1)
            got = out[at:at + size]
            at += size
            worst = max(worst, float(((got - want).abs() / want.abs()).max()))
        ok = ok and worst <= 1e-10 and bool(torch.isfinite(out).all())
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.settle_seconds:
            for f in fns.values():
                f()
            torch.cuda.synchronize()

        ms = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, f in fns.items():
                ms[name].append(timed(f, calls))
        clock = {}
        for name, f in fns.items():
            h.clock_probe(True)
            t = timed(f, calls)
            ghz, _, slots = h.clock_read()
            h.clock_probe(False)
            clock[name] = {"clock_run_ms_per_call": round(t, 4), "ghz_median": round(ghz, 4), "workgroup_slots": slots}
        med = {name: statistics.median(v) for name, v in ms.items()}
        chunks = (P + (1 << 20) - 1) >> 20
        line = {"config": config, "d": d, "n": n, "axis_length": L, "points": P, "chunks": chunks,
                "tables": len(keeps), "table_values": sum(sizes), "calls_per_round": calls,
                "worst_relative_difference_from_fp64_torch": worst,
                "ms_per_call": {name: [round(t, 4) for t in v] for name, v in ms.items()},
                "median_ms": {name: round(t, 4) for name, t in med.items()},
                "marginals_over_grid": round(med["marginals"] / med["grid"], 4),
                "added_us_per_chunk": round((med["marginals"] - med["grid"]) / chunks * 1e3, 2),
                "clock": clock}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
        del h, flow, chain
    if not ok:
        raise SystemExit("marginal tables differ from the float64 reduction of the grid values")


if __name__ == "__main__":
    main()
