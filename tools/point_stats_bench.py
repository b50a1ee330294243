"""Timing of the posterior-summary call df_flow_point_stats.

    python tools/point_stats_bench.py [--configs cfg1,cfg2,cfg4] [--points 1024] [--draws 1024]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/point_stats_bench.py --only point_stats ...

Per config (bench.py's models: cfg1 = the README chain, cfg2 = the headline chain, cfg4 = the
hidden-256 chain), M points × N draws, the legs below run interleaved in every round, each call
timed with device events after a warm-up and bench.py's settle policy (untimed rounds until
0.3 s have passed):
  (a) point_stats (ranks and sums), sbc_ranks (ranks alone) and sums (sums alone), beside their
      floor sample (df_flow_sample of the same M · N samples with the per-sample θ array
      already built) and beside hpd_ranks (df_flow_hpd_ranks over the same draws: one more
      pass output, the ldj, and the base term).  What the call adds to the floor (the θ
      repeat and the reduction kernel) are kernels inside it: --only LEGS runs legs alone,
      untimed, for a kernel-trace run of its own.
  (b) host_route: the loop the call replaces — sample(flow, N, θ_i) per point, read back,
      counted and averaged with numpy — by the wall clock, beside point_stats' wall clock
      including the read-back of the ranks and the sums.
Prints one JSON line per config: median ms per call with the range, the ratios, the bytes the
reduction kernel reads (4 · d per sample) and the effective shader clock of the forward pass
(df_chain_clock_probe).
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3, help="repetitions of the host route")
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
    from densityflows_amd.flows import moments_from_sums

    if not torch.cuda.is_available():
        raise SystemExit("point_stats_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    M, N = args.points, args.draws
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
        rank = torch.empty(M * d, dtype=torch.int32, device=dev)
        sums = torch.empty(M * S, dtype=torch.float64, device=dev)
        hrank = torch.empty(M, dtype=torch.int32, device=dev)
        seed = 7

        def call_wall():
            h.run_point_stats(x, th, M, N, 0, seed, 0, rank, sums)
            return rank.cpu().numpy().reshape(M, d), sums.cpu().numpy().reshape(M, S)

        def host_route():
            ranks = np.empty((M, d), np.int32)
            mean = np.empty((M, d))
            cov = np.empty((M, d, d))
            for i in range(M):
                q = dfa.sample(flow, N, tuple(float(v) for v in thh[:, i]) if n else None, seed=seed,
                               offset=i * d * N // 4)
                q = q.cpu().numpy() if hasattr(q, "cpu") else np.asarray(q)
                ranks[i] = np.count_nonzero(q < xh[:, i:i + 1], axis=1)
                q64 = q.astype(np.float64)
                mean[i] = q64.mean(axis=1)
                cov[i] = np.cov(q64)
            return ranks, mean, cov

        legs = {"point_stats": lambda: h.run_point_stats(x, th, M, N, 0, seed, 0, rank, sums),
                "sbc_ranks": lambda: h.run_point_stats(x, th, M, N, 0, seed, 0, rank, None),
                "sums": lambda: h.run_point_stats(None, th, M, N, 0, seed, 0, None, sums),
                "sample": lambda: h.run_sample(xs, th_rep, False, M * N, seed, 0),
                "hpd_ranks": lambda: h.run_hpd_ranks(x, th, M, N, 0, seed, 0, hrank)}
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
        res = {"config": cfg, "points": M, "draws": N, "d": d, "n": n, "calls": args.calls, "settle_rounds": settle,
               "interleaved": list(legs), "reduction_read_bytes": 4 * d * M * N}
        med = {}
        for name, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            med[name] = statistics.median(ms)
            res[name] = {"ms_median": round(med[name], 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        res["point_stats"]["msamples_per_s"] = round(M * N / med["point_stats"] / 1e3, 2)
        # (b) by the wall clock, interleaved; the two routes must agree
        wall = {"point_stats": [], "host_route": []}
        same_ranks, mean_gap, cov_gap = True, 0.0, 0.0
        for _ in range(args.host_calls):
            for name, fn in (("point_stats", call_wall), ("host_route", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "point_stats":
                    ref_r = r[0]
                    ref_mean, ref_cov = moments_from_sums(r[1], d, N)
                else:
                    same_ranks = same_ranks and bool(np.array_equal(r[0], ref_r))
                    mean_gap = max(mean_gap, float(np.max(np.abs(r[1].T - ref_mean))))
                    cov_gap = max(cov_gap, float(np.max(np.abs(np.moveaxis(r[2], 0, -1) - ref_cov))))
        for name, ms in wall.items():
            res.setdefault(name, {}).update({"wall_ms_median": round(statistics.median(ms), 4),
                                             "wall_ms_min": round(min(ms), 4), "wall_ms_max": round(max(ms), 4)})
        res["host_route_same_ranks"] = same_ranks
        res["host_route_max_abs_gap"] = {"mean": mean_gap, "cov": cov_gap}
        res["ratios"] = {k + "/sample": round(med[k] / med["sample"], 4) for k in ("point_stats", "sbc_ranks", "sums",
                                                                                   "hpd_ranks")}
        res["ratios"]["point_stats/hpd_ranks"] = round(med["point_stats"] / med["hpd_ranks"], 4)
        res["ratios"]["host_route/point_stats(wall)"] = round(
            statistics.median(wall["host_route"]) / statistics.median(wall["point_stats"]), 2)
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
