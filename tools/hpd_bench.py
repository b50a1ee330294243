"""Timing of the calibration call df_flow_hpd_ranks.

    python tools/hpd_bench.py [--configs cfg1,cfg2,cfg4] [--points 1024] [--draws 1024]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/hpd_bench.py --only hpd_ranks ...

Per config (bench.py's models: cfg1 = the README chain, cfg2 = the headline chain, cfg4 = the
hidden-256 chain), M points × N draws, the legs below run interleaved in every round, each call
timed with device events after a warm-up and bench.py's settle policy (untimed rounds until
0.3 s have passed):
  (a) hpd_ranks (df_flow_hpd_ranks, ranks alone) beside its floor sample_logpdf
      (df_flow_sample_logpdf of the same M · N samples with the per-sample θ array already
      built), and points_logpdf (df_flow_logpdf of the M points), one of the three parts the
      call adds to the floor.  The other two (the θ repeat, and the count kernel in
      sub_ldj_kernel's place) are kernels inside the call: --only LEG runs one leg alone,
      untimed, for a kernel-trace run of its own.
  (b) host_route: the loop the call replaces — sample_logpdf(flow, N, θ_i) per point, the lp
      read back, counted on the host against logpdf(flow, x, θ) — by the wall clock, beside
      hpd_ranks' wall clock including the read-back of the M ranks.
Prints one JSON line per config: median ms per call with the range, the ratios, and the
effective shader clock of the forward pass (df_chain_clock_probe).
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

    if not torch.cuda.is_available():
        raise SystemExit("hpd_bench needs an MI355X: no HIP device visible")
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
        xs = torch.empty(M * N * d, dtype=torch.float32, device=dev)
        lps = torch.empty(M * N, dtype=torch.float32, device=dev)
        lp = torch.empty(M, dtype=torch.float32, device=dev)
        rank = torch.empty(M, dtype=torch.int32, device=dev)
        seed = 7

        def hpd_wall():
            h.run_hpd_ranks(x, th, M, N, 0, seed, 0, rank)
            return rank.cpu().numpy()

        def host_route():
            lpp = dfa.logpdf(flow, xh, thh if n else None)
            out = np.empty(M, np.int32)
            for i in range(M):
                _, q = dfa.sample_logpdf(flow, N, tuple(float(v) for v in thh[:, i]) if n else None, seed=seed,
                                         offset=i * d * N // 4)
                out[i] = np.count_nonzero(q.cpu().numpy() > lpp[i])
            return out

        legs = {"hpd_ranks": lambda: h.run_hpd_ranks(x, th, M, N, 0, seed, 0, rank),
                "sample_logpdf": lambda: h.run_sample_logpdf(xs, lps, th_rep, False, M * N, seed, 0),
                "points_logpdf": lambda: h.run_logpdf(x, th, lp, M)}
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
               "interleaved": list(legs)}
        med = {}
        for name, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            med[name] = statistics.median(ms)
            res[name] = {"ms_median": round(med[name], 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        res["hpd_ranks"]["msamples_per_s"] = round(M * N / med["hpd_ranks"] / 1e3, 2)
        # (b) by the wall clock, interleaved; the two routes must count the same
        wall = {"hpd_ranks": [], "host_route": []}
        same = True
        for _ in range(args.host_calls):
            for name, fn in (("hpd_ranks", hpd_wall), ("host_route", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "hpd_ranks":
                    ref = r
                else:
                    same = same and bool(np.array_equal(r, ref))
        for name, ms in wall.items():
            res.setdefault(name, {}).update({"wall_ms_median": round(statistics.median(ms), 4),
                                             "wall_ms_min": round(min(ms), 4), "wall_ms_max": round(max(ms), 4)})
        res["host_route_same_ranks"] = same
        res["ratios"] = {"hpd_ranks/sample_logpdf": round(med["hpd_ranks"] / med["sample_logpdf"], 4),
                         "(hpd_ranks-sample_logpdf)/points_logpdf": round(
                             (med["hpd_ranks"] - med["sample_logpdf"]) / med["points_logpdf"], 4),
                         "host_route/hpd_ranks(wall)": round(
                             statistics.median(wall["host_route"]) / statistics.median(wall["hpd_ranks"]), 2)}
        h.clock_probe(True)
        for _ in range(5):
            legs["sample_logpdf"]()
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
