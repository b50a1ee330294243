"""Timing of sampling with densities and of the moment reductions.

    python tools/moments_bench.py [--configs cfg2,cfg1,cfg4] [--batch 1048576] [--wide-batch 262144]

Per config (bench.py's models: cfg2 = the headline chain, cfg1 = the README chain, cfg4 = the
hidden-256 chain) the legs below run interleaved in every round, each call timed with
device events after a warm-up and bench.py's settle policy (untimed rounds until 0.3 s have
passed):
  (a) sample (df_flow_sample), sample_logpdf (df_flow_sample_logpdf), flow_logpdf
      (df_flow_logpdf on the drawn points; sample + flow_logpdf is the pair the new call
      replaces)
  (b) logpdf_grad (df_train_logpdf_grad writing lp and gθ, no ∂x) and score_moments
      (df_train_score_moments) on the same points          — fused-sweep chains only
  (c) fisher (df_train_fisher) beside host_fisher: draw + logpdf_grad + device-to-host copy
      of lp and gθ + the numpy sums; both also by the wall clock (host_fisher's sums run on
      the host, outside any event pair)                     — fused-sweep chains only
  (d) entropy (df_flow_sample_logpdf_moments), every chain class
Prints one JSON line per config: median ms per call, the ratios, and the effective shader
clock of the forward pass (df_chain_clock_probe).
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
    ap.add_argument("--configs", default="cfg2,cfg1,cfg4")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--wide-batch", type=int, default=1 << 18, help="samples at cfg4")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import bench
    from densityflows_amd import _lib
    from densityflows_amd.train import Adam, HIPTrainer

    if not torch.cuda.is_available():
        raise SystemExit("moments_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    for cfg in args.configs.split(","):
        h = bench.build_chain(cfg).hip()
        d, n = h.d, h.n
        B = args.wide_batch if cfg == "cfg4" else args.batch
        if n:
            h.set_theta_bounds(np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32))
        tr = None
        try:
            tr = HIPTrainer(h, Adam())
            if tr.sweep() != 1:          # DF_SWEEP_FUSED
                tr.close()
                tr = None
        except _lib.UnsupportedError:
            tr = None
        thvec = torch.full((n,), 1.25, dtype=torch.float32, device=dev) if n else None
        th = torch.full((B * n,), 1.25, dtype=torch.float32, device=dev) if n else None
        x = torch.empty(B * d, dtype=torch.float32, device=dev)
        x2 = torch.empty(B * d, dtype=torch.float32, device=dev)
        lp = torch.empty(B, dtype=torch.float32, device=dev)
        gth = torch.empty(B * n, dtype=torch.float32, device=dev) if n else None
        E = 3 + n + n * n
        out = torch.empty(E, dtype=torch.float64, device=dev)
        seed = 7

        def host_fisher():
            h.run_sample(x2, thvec, True, B, seed, 0)
            tr.logpdf_grad(x2, th, B, lp, None, gth)
            l = lp.cpu().numpy().astype(np.float64)
            blk = [float(B), l.sum(), (l * l).sum()]
            if n:
                g = gth.cpu().numpy().astype(np.float64).reshape(B, n)
                blk += list(g.sum(axis=0)) + list((g.T @ g).ravel())
            return blk

        legs = {"sample": lambda: h.run_sample(x, thvec, True, B, seed, 0),
                "sample_logpdf": lambda: h.run_sample_logpdf(x2, lp, thvec, True, B, seed, 0),
                "flow_logpdf": lambda: h.run_logpdf(x, th, lp, B),
                "entropy": lambda: h.run_sample_logpdf_moments(thvec, B, 0, seed, 0, out[:3])}
        if tr is not None:
            legs.update({"logpdf_grad": lambda: tr.logpdf_grad(x, th, B, lp, None, gth),
                         "score_moments": lambda: tr.score_moments(x, th, B, out),
                         "fisher": lambda: tr.fisher(thvec, B, out, 0, seed, 0),
                         "host_fisher": host_fisher})

        def round_(times=None, wall=None):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if wall is not None and name in wall:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                if wall is not None and name in wall:
                    torch.cuda.synchronize()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
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
        wall = {k: [] for k in ("fisher", "host_fisher") if k in legs}
        for _ in range(args.calls):
            round_(times, wall)
        torch.cuda.synchronize()
        res = {"config": cfg, "batch": B, "d": d, "n": n, "calls": args.calls, "settle_rounds": settle,
               "interleaved": list(legs)}
        med = {}
        for name, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            med[name] = statistics.median(ms)
            res[name] = {"ms_median": round(med[name], 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                         "msamples_per_s": round(B / med[name] / 1e3, 2)}
        for name, ms in wall.items():
            res[name]["wall_ms_median"] = round(statistics.median(ms), 4)
        pair = med["sample"] + med["flow_logpdf"]
        res["ratios"] = {"sample_logpdf/sample": round(med["sample_logpdf"] / med["sample"], 4),
                         "sample_logpdf/(sample+flow_logpdf)": round(med["sample_logpdf"] / pair, 4),
                         "entropy/sample_logpdf": round(med["entropy"] / med["sample_logpdf"], 4)}
        if tr is not None:
            res["ratios"]["score_moments/logpdf_grad"] = round(med["score_moments"] / med["logpdf_grad"], 4)
            res["ratios"]["fisher/host_fisher(wall)"] = round(
                statistics.median(wall["fisher"]) / statistics.median(wall["host_fisher"]), 4)
            res["fisher_ns_per_sample"] = round(statistics.median(wall["fisher"]) * 1e6 / B, 3)
            res["host_fisher_ns_per_sample"] = round(statistics.median(wall["host_fisher"]) * 1e6 / B, 3)
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
        if tr is not None:
            tr.close()


if __name__ == "__main__":
    main()
