"""Timing of the weighted quantile and histogram calls df_draw_weighted_quantiles /
df_draw_weighted_histograms.

    python tools/wquant_bench.py [--dims 5,32] [--points 1024] [--draws 1024] [--split-draws 1048576]

Per d, M points × N synthetic draws (standard normal) under lognormal weights (σ = --sigma), six
probabilities and the corner at --bins bins per dimension; and, as "split", one point of
--split-draws draws at the first d for the tables.  The device legs run interleaved in every round,
each call timed with device events after a warm-up and bench.py's settle policy:
  wquantiles   (1) df_draw_weighted_quantiles            whist       (1) df_draw_weighted_histograms
  quantiles    (2) df_order_statistics, same draws       hist        (2) df_draw_histograms, same draws
  resample     (3) df_draw_resample with K = N (systematic); the route the new calls replace on the
               device is resample + quantiles and resample + hist
  scale            df_draw_weight_scale alone: the part of (1) that only reads the weights
and by the wall clock, with the read-back, for the first --host-points points:
  numpy        (4) np.quantile(weights=q, method="inverted_cdf") per dimension, and
               np.histogram(weights=) / np.histogram2d(weights=) per table
Prints one JSON line per setting: median ms per call with the range, the ratios, and the effective
shader clock of a forward pass of bench.py's config-1 chain right after the legs
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

from tools.histograms_bench import _corner, _emit, _stats, _timed  # noqa: E402


def _numpy_route(x, w, probs, edges, keep):
    """The host route of (4) on numpy draws (P, N, d) and float64 weights (P, N)."""
    for i in range(x.shape[0]):
        for k in range(x.shape[2]):
            np.quantile(x[i, :, k].astype(np.float64), probs, weights=w[i], method="inverted_cdf")
        for K in keep:
            if len(K) == 1:
                np.histogram(x[i, :, K[0]], edges[K[0]], weights=w[i])
            else:
                np.histogram2d(x[i, :, K[0]], x[i, :, K[1]], (edges[K[0]], edges[K[1]]), weights=w[i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="5,32")
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--lo", type=float, default=-4.0)
    ap.add_argument("--hi", type=float, default=4.0)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--split-draws", type=int, default=1 << 20, help="draws of the one-point table setting (0: skip)")
    ap.add_argument("--host-points", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import bench
    import densityflows_amd as dfa
    from densityflows_amd import hip
    from densityflows_amd.data import MetaData

    if not torch.cuda.is_available():
        raise SystemExit("wquant_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    probs = (0.025, 0.16, 0.5, 0.5, 0.84, 0.975)
    nums = dfa.quantile_numerators(probs)
    chain = bench.build_chain("cfg1")
    n = chain.hip().n
    clock_chain = dfa.Flow(chain, metadata=MetaData("", chain.hip().d, n, np.full(n, -1.0, np.float32),
                                                    np.full(n, 3.0, np.float32))).hip()

    def clock():
        h = clock_chain
        B = 1 << 16
        xb = torch.empty(B * h.d, dtype=torch.float32, device=dev)
        th = torch.zeros(B * h.n, dtype=torch.float32, device=dev) if h.n else None
        h.clock_probe(True)
        for _ in range(5):
            h.run_sample(xb, th, False, B, 7, 0)
        torch.cuda.synchronize()
        med, mean, slots = h.clock_read()
        h.clock_probe(False)
        return {"median": round(med, 4), "mean": round(mean, 4), "slots": slots}

    dims = [int(v) for v in args.dims.split(",")]
    settings = [("points", d, args.points, args.draws) for d in dims]
    if args.split_draws:
        settings.append(("split", dims[0], 1, args.split_draws))
    for kind, d, M, N in settings:
        g = torch.Generator(device=dev).manual_seed(d + N)
        xs = torch.randn((M, N, d), dtype=torch.float32, device=dev, generator=g)
        w = torch.exp(args.sigma * torch.randn((M, N), dtype=torch.float32, device=dev, generator=g))
        edges, bins = dfa.histogram_edges([(args.lo, args.hi, args.bins)] * d, d)
        keep = _corner(bins)
        T = sum(int(np.prod([bins[k] for k in K])) for K in keep)
        eb = torch.from_numpy(np.concatenate(edges)).to(dev)
        orders = sorted({int(p * (N - 1)) for p in probs})
        scale = torch.empty((M, 2), dtype=torch.int64, device=dev)
        qw = torch.empty((M, d, len(nums)), dtype=torch.float32, device=dev)
        qo = torch.empty((M, d, len(orders)), dtype=torch.float32, device=dev)
        sums = torch.empty((M, T), dtype=torch.int64, device=dev)
        counts = torch.empty((M, T), dtype=torch.int32, device=dev)
        res_x = torch.empty((M, N, d), dtype=torch.float32, device=dev)
        ws = torch.empty((M, N), dtype=torch.int64, device=dev) if N > dfa.RESAMPLE_LDS_DRAWS else None
        legs = {}
        if kind == "points":
            legs["wquantiles"] = lambda: hip.run_draw_weighted_quantiles(xs, w, d, M, N, nums, qw, scale)
            legs["quantiles"] = lambda: hip.run_order_statistics(xs, d, M, N, orders, qo)
        legs["whist"] = lambda: hip.run_draw_weighted_histograms(xs, w, d, M, N, eb, bins, keep, sums, scale)
        legs["hist"] = lambda: hip.run_draw_histograms(xs, d, M, N, eb, bins, keep, counts)
        legs["resample"] = lambda: hip.run_draw_resample(xs, w, d, M, N, N, 0, 7, 0, res_x, None, ws)
        legs["scale"] = lambda: hip.run_draw_weight_scale(w, M, N, scale)
        ms, settle = _timed(legs, args, torch)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"setting": kind, "points": M, "draws": N, "d": d, "probs": len(nums), "bins": args.bins,
               "tables": len(keep), "block_words": T, "sigma": args.sigma, "calls": args.calls,
               "settle_rounds": settle, "interleaved": list(legs), "draws_bytes_one_pass": 4 * d * M * N}
        for k, v in ms.items():
            res[k] = _stats(v)
        ratios = {"whist/hist": round(med["whist"] / med["hist"], 3),
                  "whist/(resample+hist)": round(med["whist"] / (med["resample"] + med["hist"]), 3)}
        if kind == "points":
            ratios["wquantiles/quantiles"] = round(med["wquantiles"] / med["quantiles"], 3)
            ratios["wquantiles/(resample+quantiles)"] = round(med["wquantiles"] / (med["resample"] + med["quantiles"]), 3)
            # (4) the numpy route with its read-back against the two new calls with theirs, by the wall clock
            hp = min(M, args.host_points)
            wall = {"device": [], "numpy": []}
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                legs["wquantiles"]()
                legs["whist"]()
                qw.cpu(), sums.cpu(), scale.cpu()
                wall["device"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                xh, wh = xs[:hp].cpu().numpy(), w[:hp].cpu().numpy().astype(np.float64)
                _numpy_route(xh, wh, probs, edges, keep)
                wall["numpy"].append((time.perf_counter() - t0) * 1e3)
            res["wall_ms"] = {"device_all_points": round(statistics.median(wall["device"]), 3),
                              "numpy": round(statistics.median(wall["numpy"]), 3), "numpy_points": hp}
            ratios["numpy_per_point/device_per_point"] = round(
                (statistics.median(wall["numpy"]) / hp) / (statistics.median(wall["device"]) / M), 1)
        res["ratios"] = ratios
        res["forward_pass_clock_ghz"] = clock()
        _emit(res, args)


if __name__ == "__main__":
    main()
