"""Timing of the posterior-quantile calls df_flow_point_quantiles / df_order_statistics.

    python tools/quantiles_bench.py [--configs cfg1,cfg2,cfg4] [--points 1024] [--draws 1024]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/quantiles_bench.py --only select ...

Per config (bench.py's models: cfg1 = the README chain, cfg2 = the headline chain, cfg4 = the
hidden-256 chain), M points × N draws and the orders of probs = (0.16, 0.5, 0.84) (six at
N = 1024), the legs below run interleaved in every round, each call timed with device events
after a warm-up and bench.py's settle policy (untimed rounds until 0.3 s have passed):
  quantiles        (i)   df_flow_point_quantiles, quant_out alone
  quantiles_stats  (ii)  the same with rank_out and sums_out
  point_stats      (iii) df_flow_point_stats with rank_out and sums_out (the yardstick)
  sample           (iv)  df_flow_sample of the same M · N samples, per-sample θ already built
  select           (v)   df_order_statistics alone, over the samples of (iv)
and by the wall clock, interleaved, --host-calls times:
  quantiles (wall)       (i) with the read-back of its d · M · Q floats
  host_route       (vi)  the path it replaces: df_flow_point_stats with draws_out alone, the
                         read-back of d · M · N floats, np.partition at the same orders
The two routes must agree bit for bit.  Prints one JSON line per config: median ms per call
with the range, the ratios, the bytes each route moves to the host and the effective shader
clock of the forward pass (df_chain_clock_probe).  --only LEGS runs legs alone, untimed, for a
kernel-trace run of its own.
"""
import argparse
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
    ap.add_argument("--configs", default="cfg1,cfg2,cfg4")
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--probs", default="0.16,0.5,0.84")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3, help="repetitions of the two wall-clock routes")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-seconds", type=float, default=0.3)
    ap.add_argument("--only", default=None,
                    help="run these legs (comma-separated) alone, --calls times, untimed (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import bench
    import densityflows_amd as dfa
    from densityflows_amd.data import MetaData
    from densityflows_amd.hip import run_order_statistics

    if not torch.cuda.is_available():
        raise SystemExit("quantiles_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    M, N = args.points, args.draws
    orders, _, _, _ = dfa.quantile_orders([float(v) for v in args.probs.split(",")], N)
    orders = [int(v) for v in orders]
    Q = len(orders)
    for cfg in args.configs.split(","):
        chain = bench.build_chain(cfg)
        h0 = chain.hip()
        d, n = h0.d, h0.n
        flow = dfa.Flow(chain, metadata=MetaData("", d, n, np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32)))
        h = flow.hip()
        rng = np.random.default_rng(1)
        xh = rng.standard_normal((d, M)).astype(np.float32)
        thh = rng.uniform(-1, 3, (n, M)).astype(np.float32)
        flat = lambda a: torch.from_numpy(np.ascontiguousarray(a.T).ravel()).to(dev)
        x = flat(xh)
        th = flat(thh) if n else None
        th_rep = flat(np.repeat(thh, N, axis=1)) if n else None
        S = 2 * d + d * (d + 1) // 2
        xs = torch.empty(M * N * d, dtype=torch.float32, device=dev)
        draws = torch.empty(M * N * d, dtype=torch.float32, device=dev)
        quant = torch.empty(M * d * Q, dtype=torch.float32, device=dev)
        quant2 = torch.empty(M * d * Q, dtype=torch.float32, device=dev)
        rank = torch.empty(M * d, dtype=torch.int32, device=dev)
        sums = torch.empty(M * S, dtype=torch.float64, device=dev)
        seed = 7

        def call_wall():
            h.run_point_quantiles(None, th, M, N, 0, seed, 0, orders, quant)
            return quant.cpu().numpy().reshape(M, d, Q)

        def host_route():
            h.run_point_stats(None, th, M, N, 0, seed, 0, None, None, draws)
            q = draws.cpu().numpy().reshape(M, N, d)
            return np.ascontiguousarray(np.partition(q, sorted(set(orders)), axis=1)[:, orders, :].transpose(0, 2, 1))

        legs = {"quantiles": lambda: h.run_point_quantiles(None, th, M, N, 0, seed, 0, orders, quant),
                "quantiles_stats": lambda: h.run_point_quantiles(x, th, M, N, 0, seed, 0, orders, quant, rank, sums),
                "point_stats": lambda: h.run_point_stats(x, th, M, N, 0, seed, 0, rank, sums),
                "sample": lambda: h.run_sample(xs, th_rep, False, M * N, seed, 0),
                "select": lambda: run_order_statistics(xs, d, M, N, orders, quant2)}
        legs["sample"]()                     # select reads these samples, whatever runs first
        if args.only:
            for _ in range(args.warmup + args.calls):
                for name in args.only.split(","):
                    legs[name]()
            torch.cuda.synchronize()
            continue

        def round_(times=None):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                if times is not None:
                    times[name].append((e0, e1))

        t_warm = time.perf_counter()
        for _ in range(args.warmup):
            round_()
        torch.cuda.synchronize()
        settle = 0
        while time.perf_counter() - t_warm < args.settle_seconds and settle < 10000:
            round_()
            torch.cuda.synchronize()
            settle += 1
        times = {k: [] for k in legs}
        for _ in range(args.calls):
            round_(times)
        torch.cuda.synchronize()
        res = {"config": cfg, "points": M, "draws": N, "d": d, "n": n, "orders": orders, "calls": args.calls,
               "settle_rounds": settle, "interleaved": list(legs), "selection_read_bytes_per_pass": 4 * d * M * N,
               "host_bytes": {"quantiles": 4 * d * M * Q, "host_route": 4 * d * M * N}}
        med = {}
        for name, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            med[name] = statistics.median(ms)
            res[name] = {"ms_median": round(med[name], 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        # the two routes by the wall clock, interleaved; they must agree bit for bit
        wall = {"quantiles": [], "host_route": []}
        same = True
        for _ in range(args.host_calls):
            for name, fn in (("quantiles", call_wall), ("host_route", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "quantiles":
                    ref = r
                else:
                    same = same and bool(np.array_equal(r.view(np.uint32), ref.view(np.uint32)))
        for name, ms in wall.items():
            res.setdefault(name, {}).update({"wall_ms_median": round(statistics.median(ms), 4),
                                             "wall_ms_min": round(min(ms), 4), "wall_ms_max": round(max(ms), 4)})
        res["host_route_same_bits"] = same
        spread = max(max(ms) - min(ms) for ms in wall.values())
        gap = statistics.median(wall["host_route"]) - statistics.median(wall["quantiles"])
        res["wall_gap_ms"] = round(gap, 4)
        res["wall_spread_ms"] = round(spread, 4)
        res["quantiles_beat_host_route"] = bool(gap > spread)
        res["ratios"] = {k + "/sample": round(med[k] / med["sample"], 4)
                         for k in ("quantiles", "quantiles_stats", "point_stats", "select")}
        res["ratios"]["quantiles_stats/point_stats"] = round(med["quantiles_stats"] / med["point_stats"], 4)
        res["ratios"]["host_route/quantiles(wall)"] = round(
            statistics.median(wall["host_route"]) / statistics.median(wall["quantiles"]), 2)
        h.clock_probe(True)
        for _ in range(5):
            legs["sample"]()
        torch.cuda.synchronize()
        ghz_med, ghz_mean, slots = h.clock_read()
        h.clock_probe(False)
        res["forward_pass_clock_ghz"] = {"median": round(ghz_med, 4), "mean": round(ghz_mean, 4), "slots": slots}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
