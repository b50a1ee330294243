"""Timing of the resampling call df_draw_resample.

    python tools/resample_bench.py [--shapes cfg1:1024:1024:1024,cfg4:1024:1024:1024,cfg1:1:1048576:1048576]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/resample_bench.py --only systematic ...

Per shape ``config:M:N:K`` (bench.py's models: cfg1 = the README chain, d = 5; cfg4 = the
hidden-256 chain, d = 32), M points × N draws made once by df_flow_sample_logpdf with θ repeated
per point, a synthetic unnormalised Gaussian as the target and df_importance_weights' own weights.
One point of 2^20 draws takes the two-kernel path (the scan in cdf_ws, the picks over the device).
The legs below run interleaved in every round, each call timed with device events after a warm-up
and bench.py's settle policy (untimed rounds until 0.3 s have passed):
  systematic, stratified, multinomial   df_draw_resample, picks and gathered rows, K picks per point
  systematic_idx                        the same without the gather (xs_out = NULL)
  weighted                              df_draw_weighted_stats, sums only, on the same draws and
                                        weights: the neighbour that reads the same arrays
and by the wall clock, interleaved, --host-calls times:
  device_route   the systematic call with the read-back of the M·K·d floats
  host_route     the path it replaces: read back the draws and the weights, then per point numpy's
                 cumsum / searchsorted / take (float64 systematic resampling).  --host-points P
                 resamples the first P points only (the read-back stays whole)
The byte floor of a call is 4N + 8Kd + 4K bytes per point: the weights read, the picked rows read
and written, the index store.  Prints one JSON line per shape: median ms per call with the range,
the floor's share, the ratios and the effective shader clock of the forward pass
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from importance_bench import _stats, _timed  # noqa: E402  (the sibling's interleaved event timing)


def _host_resample(q, w, K, points, rng):
    """numpy per point: systematic resampling in float64 → the picked rows (P, K, d)."""
    out = np.empty((points, K, q.shape[2]), np.float32)
    for i in range(points):
        c = np.cumsum(w[i].astype(np.float64))
        u = (np.arange(K) + rng.random()) / K * c[-1]
        idx = np.minimum(np.searchsorted(c, u, side="right"), w.shape[1] - 1)
        out[i] = np.take(q[i], idx, axis=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg1:1024:1024:1024,cfg4:1024:1024:1024,cfg1:1:1048576:1048576",
                    help="comma-separated config:points:draws:picks")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3, help="repetitions of the two wall-clock routes")
    ap.add_argument("--host-points", type=int, default=0, help="points the host route resamples (0: all)")
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
    from densityflows_amd.hip import run_draw_resample, run_draw_weighted_stats, run_importance_weights

    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    codes = dfa.RESAMPLE_METHODS
    for shape in args.shapes.split(","):
        cfg, M, N, K = shape.split(":")
        M, N, K = int(M), int(N), int(K)
        chain = bench.build_chain(cfg)
        h0 = chain.hip()
        d, n = h0.d, h0.n
        flow = dfa.Flow(chain, metadata=MetaData("", d, n, np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32)))
        h = flow.hip()
        rng = np.random.default_rng(1)
        thh = rng.uniform(-1, 3, (n, M)).astype(np.float32)
        flat = lambda a: torch.from_numpy(np.ascontiguousarray(a.T).ravel()).to(dev)
        th_rep = flat(np.repeat(thh, N, axis=1)) if n else None
        seed = 7
        SW = 2 + 2 * d + d * (d + 1) // 2
        draws = torch.empty(M * N * d, dtype=torch.float32, device=dev)
        lq = torch.empty(M * N, dtype=torch.float32, device=dev)
        h.run_sample_logpdf(draws, lq, th_rep, False, M * N, seed, 0)
        lt = -0.5 * ((draws.view(M, N, d) - 0.25) ** 2).sum(dim=-1).reshape(-1)       # the target, unnormalised
        w = torch.empty(M * N, dtype=torch.float32, device=dev)
        stats = torch.empty(4 * M, dtype=torch.float64, device=dev)
        run_importance_weights(lt - lq, M, N, w, stats)
        out = torch.empty(M * K * d, dtype=torch.float32, device=dev)
        idx = torch.empty(M * K, dtype=torch.int32, device=dev)
        ws = torch.empty(M * N, dtype=torch.int64, device=dev) if N > dfa.RESAMPLE_LDS_DRAWS else None
        wsums = torch.empty(SW * M, dtype=torch.float64, device=dev)
        xs = torch.empty(M * N * d, dtype=torch.float32, device=dev)

        def leg(method, gather=True):
            return lambda: run_draw_resample(draws if gather else None, w, d if gather else 0, M, N, K, codes[method],
                                             seed, 0, out if gather else None, idx, ws)

        legs = {m: leg(m) for m in codes}
        legs["systematic_idx"] = leg("systematic", False)
        legs["weighted"] = lambda: run_draw_weighted_stats(draws, w, None, d, M, N, None, wsums)
        if args.only:
            for _ in range(args.warmup + args.calls):
                for name in args.only.split(","):
                    legs[name]()
            torch.cuda.synchronize()
            continue
        ms, settle = _timed(legs, args, torch)
        med = {k: statistics.median(v) for k, v in ms.items()}
        floor = (4 * N + 8 * K * d + 4 * K) * M
        st = stats.cpu().numpy().reshape(M, 4)
        res = {"config": cfg, "points": M, "draws": N, "picks": K, "d": d, "n": n, "calls": args.calls,
               "settle_rounds": settle, "interleaved": list(legs),
               "path": "wave" if N <= 256 else "workgroup" if N <= dfa.RESAMPLE_LDS_DRAWS else "scan + pick",
               "floor_bytes": floor, "weighted_bytes_read": 4 * (d + 1) * M * N,
               "ess_median": round(float(np.median(st[:, 1] ** 2 / st[:, 2])), 2)}
        for k, v in ms.items():
            res[k] = _stats(v)
        for m in codes:
            res[m]["floor_GBps"] = round(floor / med[m] / 1e6, 1)
        res["weighted"]["read_GBps"] = round(4 * (d + 1) * M * N / med["weighted"] / 1e6, 1)
        res["ratios"] = {m + "/weighted": round(med[m] / med["weighted"], 3) for m in codes}
        res["ratios"]["systematic_idx/systematic"] = round(med["systematic_idx"] / med["systematic"], 3)
        legs["systematic"]()
        torch.cuda.synchronize()
        picks = idx.cpu().numpy().reshape(M, K)
        res["unique_fraction_median"] = round(float(np.median([len(np.unique(r)) / K for r in picks[:64]])), 4)

        # the two routes by the wall clock, interleaved
        hp = M if args.host_points <= 0 else min(M, args.host_points)

        def device_route():
            legs["systematic"]()
            return out.cpu().numpy().reshape(M, K, d)

        def host_route():
            q = draws.cpu().numpy().reshape(M, N, d)
            return _host_resample(q, w.cpu().numpy().reshape(M, N), K, hp, np.random.default_rng(seed))

        wall = {"device_route": [], "host_route": []}
        for _ in range(args.host_calls):
            for name, fn in (("device_route", device_route), ("host_route", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "device_route":
                    dm = r.astype(np.float64).mean(axis=1)
                else:
                    hm = r.astype(np.float64).mean(axis=1)
        for name, wl in wall.items():
            res[name] = {"wall_ms_median": round(statistics.median(wl), 4), "wall_ms_min": round(min(wl), 4),
                         "wall_ms_max": round(max(wl), 4)}
        res["host_route"]["points_reduced"] = hp
        res["device_route"]["host_bytes"] = 4 * M * K * d
        res["host_route"]["host_bytes"] = 4 * (d + 1) * M * N
        # (two samples of the same weighted draws: their means differ by sampling noise only)
        res["routes_mean_difference"] = float(np.abs(dm[:hp] - hm).max())
        res["ratios"]["host_route/device_route(wall)"] = round(
            statistics.median(wall["host_route"]) / statistics.median(wall["device_route"]), 2)
        h.clock_probe(True)
        for _ in range(5):
            h.run_sample(xs, th_rep, False, M * N, seed, 0)
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
