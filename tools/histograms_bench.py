"""Timing of the posterior-histogram calls df_flow_point_histograms / df_draw_histograms.

    python tools/histograms_bench.py [--configs cfg1,cfg2,cfg4,cfg2_split,sparse] [--points 1024] [--draws 1024]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/histograms_bench.py --only draw ...

Per config (bench.py's models: cfg1 = the README chain, cfg2 = the headline chain, cfg4 = the
hidden-256 chain), M points × N draws and the corner at --bins bins per dimension (15 tables at
d = 5, 528 at d = 32), the legs below run interleaved in every round, each call timed with device
events after a warm-up and bench.py's settle policy (untimed rounds until 0.3 s have passed):
  histograms   (i)   df_flow_point_histograms, counts_out alone
  sample       (ii)  df_flow_sample of the same M · N samples, per-sample θ already built
  draw         (iii) df_draw_histograms alone, over the samples of (ii): the kernel's own time
and by the wall clock, interleaved, --host-calls times:
  histograms (wall)  (i) with the read-back of its M · T counts
  host_route   (iv)  the path it replaces: df_flow_point_stats with draws_out alone, the read-back
                     of d · M · N floats, np.histogram / np.histogram2d per table and point.
                     --host-points P bins the first P points only (the read-back stays whole);
                     the time of all M points is then extrapolated and marked as such, and the
                     verdict uses the measured, smaller time
The two routes must agree bit for bit.
  cfg2_split   config 2, unconditional, --split-points (ONE) point of --split-draws draws (2^20): the split path.
               The draw leg runs once per value of --split-values (the library reads
               DF_HIST_SPLIT_DRAWS from the environment at every call), interleaved.
  sparse       no chain: --sparse-points points of 4 synthetic draws into the d = 5 corner (T words
               per point, almost all zero) beside a memset of the same M · T words — the cost of
               the LDS zero-and-flush of a mostly empty block against the store floor.
Prints one JSON line per config: median ms per call with the range, the ratios, the bytes, the
draws' read bandwidth of one pass and the effective shader clock of the forward pass
(df_chain_clock_probe).  --only LEGS runs legs alone, untimed, for a kernel-trace run of its own.
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


def _corner(bins):
    xs = [k for k in range(len(bins)) if bins[k] > 0]
    return [(a,) for a in xs] + [(a, b) for i, a in enumerate(xs) for b in xs[i + 1:]]


def _host_tables(q, edges, keep):
    """np.histogram / np.histogram2d per table and point, in the block layout."""
    out = []
    for i in range(q.shape[0]):
        row = []
        for K in keep:
            if len(K) == 1:
                row.append(np.histogram(q[i, :, K[0]], edges[K[0]])[0])
            else:
                row.append(np.histogram2d(q[i, :, K[0]], q[i, :, K[1]], (edges[K[0]], edges[K[1]]))[0].T.reshape(-1))
        out.append(np.concatenate(row))
    return np.stack(out).astype(np.int32)


def _timed(legs, args, torch):
    """Interleaved rounds of the legs → {name: [ms]} and the settle count."""
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
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in times.items()}, settle


def _stats(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def _emit(res, args):
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg1,cfg2,cfg4,cfg2_split,sparse")
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--lo", type=float, default=-4.0)
    ap.add_argument("--hi", type=float, default=4.0)
    ap.add_argument("--split-draws", type=int, default=1 << 20)
    ap.add_argument("--split-points", type=int, default=1)
    ap.add_argument("--split-values", default="1024,2048,4096,16384")
    ap.add_argument("--sparse-points", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3, help="repetitions of the two wall-clock routes")
    ap.add_argument("--host-points", type=int, default=0, help="points the host route bins (0: all)")
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
    from densityflows_amd.hip import run_draw_histograms

    if not torch.cuda.is_available():
        raise SystemExit("histograms_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    for cfg in args.configs.split(","):
        if cfg == "sparse":
            d, M, N = 5, args.sparse_points, 4
            edges, bins = dfa.histogram_edges([(args.lo, args.hi, args.bins)] * d, d)
            keep = _corner(bins)
            T = sum(int(np.prod([bins[k] for k in K])) for K in keep)
            xs = torch.randn(M * N * d, dtype=torch.float32, device=dev)
            eb = torch.from_numpy(np.concatenate(edges)).to(dev)
            counts = torch.empty(M * T, dtype=torch.int32, device=dev)
            other = torch.empty(M * T, dtype=torch.int32, device=dev)
            legs = {"draw": lambda: run_draw_histograms(xs, d, M, N, eb, bins, keep, counts),
                    "memset": lambda: other.zero_()}
            ms, settle = _timed(legs, args, torch)
            res = {"config": cfg, "points": M, "draws": N, "d": d, "tables": len(keep), "block_words": T,
                   "counts_bytes": 4 * M * T, "calls": args.calls, "settle_rounds": settle, "interleaved": list(legs)}
            for k, v in ms.items():
                res[k] = _stats(v)
                res[k]["store_GBps"] = round(4 * M * T / statistics.median(v) / 1e6, 1)
            res["ratios"] = {"draw/memset": round(statistics.median(ms["draw"]) / statistics.median(ms["memset"]), 3)}
            _emit(res, args)
            continue

        split = cfg == "cfg2_split"
        chain = bench.build_chain("cfg2" if split else cfg)
        h0 = chain.hip()
        d, n = h0.d, h0.n
        flow = dfa.Flow(chain, metadata=MetaData("", d, n, np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32)))
        h = flow.hip()
        M, N = (args.split_points, args.split_draws) if split else (args.points, args.draws)
        edges, bins = dfa.histogram_edges([(args.lo, args.hi, args.bins)] * d, d)
        keep = _corner(bins)
        T = sum(int(np.prod([bins[k] for k in K])) for K in keep)
        rng = np.random.default_rng(1)
        thh = rng.uniform(-1, 3, (n, M)).astype(np.float32)
        flat = lambda a: torch.from_numpy(np.ascontiguousarray(a.T).ravel()).to(dev)
        th = flat(thh) if n else None
        th_rep = flat(np.repeat(thh, N, axis=1)) if n else None
        eb = torch.from_numpy(np.concatenate(edges)).to(dev)
        xs = torch.empty(M * N * d, dtype=torch.float32, device=dev)
        draws = torch.empty(M * N * d, dtype=torch.float32, device=dev)
        counts = torch.empty(M * T, dtype=torch.int32, device=dev)
        counts2 = torch.empty(M * T, dtype=torch.int32, device=dev)
        seed = 7

        def call_wall():
            h.run_point_histograms(th, M, N, 0, seed, 0, eb, bins, keep, counts)
            return counts.cpu().numpy().reshape(M, T)

        hp = M if args.host_points <= 0 else min(M, args.host_points)

        def host_route():
            h.run_point_stats(None, th, M, N, 0, seed, 0, None, None, draws)
            q = draws.cpu().numpy().reshape(M, N, d)
            return _host_tables(q[:hp], edges, keep)

        def draw_at(value):
            def fn():
                if value is None:
                    os.environ.pop("DF_HIST_SPLIT_DRAWS", None)
                else:
                    os.environ["DF_HIST_SPLIT_DRAWS"] = str(value)
                run_draw_histograms(xs, d, M, N, eb, bins, keep, counts2)
                os.environ.pop("DF_HIST_SPLIT_DRAWS", None)
            return fn

        legs = {"histograms": lambda: h.run_point_histograms(th, M, N, 0, seed, 0, eb, bins, keep, counts),
                "sample": lambda: h.run_sample(xs, th_rep, False, M * N, seed, 0),
                "draw": draw_at(None)}
        if split:
            for v in args.split_values.split(","):
                legs[f"draw@{int(v)}"] = draw_at(int(v))
        legs["sample"]()                     # draw reads these samples, whatever runs first
        if args.only:
            for _ in range(args.warmup + args.calls):
                for name in args.only.split(","):
                    legs[name]()
            torch.cuda.synchronize()
            continue
        ms, settle = _timed(legs, args, torch)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"config": cfg, "points": M, "draws": N, "d": d, "n": n, "bins": args.bins, "tables": len(keep),
               "block_words": T, "split_draws": dfa.HIST_SPLIT_DRAWS, "calls": args.calls, "settle_rounds": settle,
               "interleaved": list(legs), "draws_bytes_one_pass": 4 * d * M * N,
               "host_bytes": {"histograms": 4 * M * T, "host_route": 4 * d * M * N}}
        for k, v in ms.items():
            res[k] = _stats(v)
        for k in legs:
            if k.startswith("draw"):
                res[k]["draws_read_GBps_one_pass"] = round(4 * d * M * N / med[k] / 1e6, 1)
        if split:
            same = []
            for k in legs:
                if k.startswith("draw"):
                    legs[k]()
                    torch.cuda.synchronize()
                    same.append(counts2.cpu().numpy().copy())
            res["split_values_same_bits"] = bool(all(np.array_equal(same[0], s) for s in same[1:]))
        # the two routes by the wall clock, interleaved; they must agree bit for bit
        wall = {"histograms": [], "host_route": []}
        same = True
        for _ in range(args.host_calls):
            for name, fn in (("histograms", call_wall), ("host_route", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "histograms":
                    ref = r
                else:
                    same = same and bool(np.array_equal(r, ref[:hp]))
        for name, w in wall.items():
            res.setdefault(name, {}).update({"wall_ms_median": round(statistics.median(w), 4),
                                             "wall_ms_min": round(min(w), 4), "wall_ms_max": round(max(w), 4)})
        res["host_route"]["points_binned"] = hp
        if hp < M:
            res["host_route"]["wall_ms_all_points_extrapolated"] = round(statistics.median(wall["host_route"]) * M / hp, 1)
        res["host_route_same_bits"] = same
        spread = max(max(w) - min(w) for w in wall.values())
        gap = statistics.median(wall["host_route"]) - statistics.median(wall["histograms"])
        res["wall_gap_ms"] = round(gap, 4)
        res["wall_spread_ms"] = round(spread, 4)
        res["histograms_beat_host_route"] = bool(gap > spread)
        res["ratios"] = {k + "/sample": round(med[k] / med["sample"], 4) for k in legs if k != "sample"}
        res["ratios"]["host_route/histograms(wall)"] = round(
            statistics.median(wall["host_route"]) / statistics.median(wall["histograms"]), 2)
        h.clock_probe(True)
        for _ in range(5):
            legs["sample"]()
        torch.cuda.synchronize()
        ghz_med, ghz_mean, slots = h.clock_read()
        h.clock_probe(False)
        res["forward_pass_clock_ghz"] = {"median": round(ghz_med, 4), "mean": round(ghz_mean, 4), "slots": slots}
        _emit(res, args)


if __name__ == "__main__":
    main()
