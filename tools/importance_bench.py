"""Timing of the importance-weight calls df_importance_weights / df_draw_weighted_stats.

    python tools/importance_bench.py [--configs cfg1,cfg4] [--points 1024] [--draws 1024]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/importance_bench.py --only sums,weighted ...

Per config (bench.py's models: cfg1 = the README chain, d = 5; cfg4 = the hidden-256 chain,
d = 32), M points × N draws made once by df_flow_sample_logpdf with θ repeated per point, and a
synthetic unnormalised Gaussian as the target.  The legs below run interleaved in every round,
each call timed with device events after a warm-up and bench.py's settle policy (untimed rounds
until 0.3 s have passed):
  weights        (i)   df_importance_weights alone: w_out and the four sums of every point
  weighted       (ii)  df_draw_weighted_stats alone, sums only, over those draws and weights
  weighted_rank  (ii') the same with wrank_out
  sums           (iii) df_flow_point_stats, sums only: the draw, the forward pass and
                       point_stats_kernel — the yardstick's kernel has no entry of its own
  sample         (iv)  df_flow_sample of the same M · N samples with the per-sample θ already
                       built: the floor of (iii).  (iii) − (iv) is point_stats_kernel and the θ
                       repeat; --only LEGS runs legs alone, untimed, for a kernel-trace run of its
                       own, which times the two reduction kernels themselves
and by the wall clock, interleaved, --host-calls times:
  device_route   (i) + (ii') with the read-back of the 4 + d + 2 + 2d + d(d+1)/2 doubles per point
  host_route     (v)   the path they replace: read back the draws, log q and the target, then
                       per point exp and the weighted mean, covariance and CDF value with numpy.
                       --host-points P reduces the first P points only (the read-back stays whole)
The two routes must agree (means and log Ẑ to 1e-5: the host exponentiates in float64, the device
in Float32).
Prints one JSON line per config: median ms per call with the range, the ratios, the bytes each
kernel reads and the effective shader clock of the forward pass (df_chain_clock_probe).
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


def _host_moments(q, lq, lt, x, points):
    """numpy per point: exp of the stabilised log-weights, the weighted mean, covariance (the
    reliability-weights correction) and CDF value → (mean (P, d), cov (P, d, d), cdf (P, d),
    log Ẑ (P,), ESS (P,))."""
    d = q.shape[2]
    mean, cov, cdf = np.empty((points, d)), np.empty((points, d, d)), np.empty((points, d))
    lz, ess = np.empty(points), np.empty(points)
    for i in range(points):
        lw = (lt[i] - lq[i]).astype(np.float64)
        m = lw.max()
        w = np.exp(lw - m)
        w1, w2 = w.sum(), (w * w).sum()
        v = q[i].astype(np.float64)
        mu = w @ v / w1
        r = v - mu
        mean[i], cov[i] = mu, (r * w[:, None]).T @ r / (w1 - w2 / w1)
        cdf[i] = ((q[i] < x[:, i]) * w[:, None]).sum(axis=0) / w1
        lz[i], ess[i] = m + np.log(w1 / w.size), w1 * w1 / w2
    return mean, cov, cdf, lz, ess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg1,cfg4")
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=3, help="repetitions of the two wall-clock routes")
    ap.add_argument("--host-points", type=int, default=0, help="points the host route reduces (0: all)")
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
    from densityflows_amd.hip import run_draw_weighted_stats, run_importance_weights

    if not torch.cuda.is_available():
        raise SystemExit("importance_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    M, N = args.points, args.draws
    for cfg in args.configs.split(","):
        chain = bench.build_chain(cfg)
        h0 = chain.hip()
        d, n = h0.d, h0.n
        flow = dfa.Flow(chain, metadata=MetaData("", d, n, np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32)))
        h = flow.hip()
        rng = np.random.default_rng(1)
        thh = rng.uniform(-1, 3, (n, M)).astype(np.float32)
        xh = rng.standard_normal((d, M)).astype(np.float32)
        flat = lambda a: torch.from_numpy(np.ascontiguousarray(a.T).ravel()).to(dev)
        th = flat(thh) if n else None
        th_rep = flat(np.repeat(thh, N, axis=1)) if n else None
        xb = flat(xh)
        seed = 7
        S, SW = 2 * d + d * (d + 1) // 2, 2 + 2 * d + d * (d + 1) // 2
        draws = torch.empty(M * N * d, dtype=torch.float32, device=dev)
        lq = torch.empty(M * N, dtype=torch.float32, device=dev)
        h.run_sample_logpdf(draws, lq, th_rep, False, M * N, seed, 0)
        lt = -0.5 * ((draws.view(M, N, d) - 0.25) ** 2).sum(dim=-1).reshape(-1)       # the target, unnormalised
        logw = lt - lq
        w = torch.empty(M * N, dtype=torch.float32, device=dev)
        stats = torch.empty(4 * M, dtype=torch.float64, device=dev)
        wsums = torch.empty(SW * M, dtype=torch.float64, device=dev)
        wsums2 = torch.empty(SW * M, dtype=torch.float64, device=dev)
        wrank = torch.empty(d * M, dtype=torch.float64, device=dev)
        sums = torch.empty(S * M, dtype=torch.float64, device=dev)
        xs = torch.empty(M * N * d, dtype=torch.float32, device=dev)

        legs = {"weights": lambda: run_importance_weights(logw, M, N, w, stats),
                "weighted": lambda: run_draw_weighted_stats(draws, w, None, d, M, N, None, wsums),
                "weighted_rank": lambda: run_draw_weighted_stats(draws, w, xb, d, M, N, wrank, wsums2),
                "sums": lambda: h.run_point_stats(None, th, M, N, 0, seed, 0, None, sums),
                "sample": lambda: h.run_sample(xs, th_rep, False, M * N, seed, 0)}
        legs["weights"]()                    # the weighted legs read these weights, whatever runs first
        if args.only:
            for _ in range(args.warmup + args.calls):
                for name in args.only.split(","):
                    legs[name]()
            torch.cuda.synchronize()
            continue
        ms, settle = _timed(legs, args, torch)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"config": cfg, "points": M, "draws": N, "d": d, "n": n, "calls": args.calls, "settle_rounds": settle,
               "interleaved": list(legs),
               "bytes_read": {"weights": 2 * 4 * M * N, "weighted": 4 * (d + 1) * M * N, "point_stats_kernel": 4 * d * M * N},
               "bytes_written": {"weights": 4 * M * N + 32 * M, "weighted": 8 * SW * M},
               "host_bytes": {"device_route": 8 * (4 + d + SW) * M, "host_route": 4 * (d + 2) * M * N}}
        for k, v in ms.items():
            res[k] = _stats(v)
        res["weights"]["GBps"] = round((2 * 4 * M * N + 4 * M * N) / med["weights"] / 1e6, 1)
        res["weighted"]["read_GBps"] = round(4 * (d + 1) * M * N / med["weighted"] / 1e6, 1)
        kernel = med["sums"] - med["sample"]          # point_stats_kernel and the θ repeat
        res["sums_minus_sample_ms"] = round(kernel, 4)
        res["ratios"] = {"weighted/(sums-sample)": round(med["weighted"] / kernel, 3) if kernel > 0 else None,
                         "weighted_rank/weighted": round(med["weighted_rank"] / med["weighted"], 3),
                         "weights/sample": round(med["weights"] / med["sample"], 4),
                         "weighted/sample": round(med["weighted"] / med["sample"], 4)}

        # the two routes by the wall clock, interleaved
        hp = M if args.host_points <= 0 else min(M, args.host_points)

        def device_route():
            run_importance_weights(logw, M, N, w, stats)
            run_draw_weighted_stats(draws, w, xb, d, M, N, wrank, wsums2)
            st, blk, rk = stats.cpu().numpy().reshape(M, 4), wsums2.cpu().numpy(), wrank.cpu().numpy().reshape(M, d)
            mean, cov, ess = dfa.weighted_moments_from_sums(blk, d)
            return mean.T, np.moveaxis(cov, -1, 0), rk / blk.reshape(M, SW)[:, :1], st[:, 0] + np.log(st[:, 1] / N), ess

        def host_route():
            q = draws.cpu().numpy().reshape(M, N, d)
            return _host_moments(q, lq.cpu().numpy().reshape(M, N), lt.cpu().numpy().reshape(M, N), xh, hp)

        wall = {"device_route": [], "host_route": []}
        worst = 0.0
        for _ in range(args.host_calls):
            for name, fn in (("device_route", device_route), ("host_route", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "device_route":
                    ref = r
                else:
                    scale = np.abs(r[0]).max()
                    worst = max(worst, float(np.abs(r[0] - ref[0][:hp]).max() / scale),
                                float(np.abs(r[3] - ref[3][:hp]).max()))
        for name, wl in wall.items():
            res[name] = {"wall_ms_median": round(statistics.median(wl), 4), "wall_ms_min": round(min(wl), 4),
                         "wall_ms_max": round(max(wl), 4)}
        res["host_route"]["points_reduced"] = hp
        if hp < M:
            res["host_route"]["note"] = "the read-back is whole, the numpy reduction covers points_reduced points"
        res["routes_worst_difference"] = worst
        res["routes_agree"] = bool(worst <= 1e-5)
        res["ratios"]["host_route/device_route(wall)"] = round(
            statistics.median(wall["host_route"]) / statistics.median(wall["device_route"]), 2)
        ess = ref[4]
        res["ess_median"] = round(float(np.median(ess)), 2)
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
