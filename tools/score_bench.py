"""Timing of df_train_logpdf_grad beside df_train_gradient.

    python tools/score_bench.py [--configs cfg2,cfg1] [--batch 1048576] [--calls 20]

Per config (bench.py's models: cfg2 = the headline chain, cfg1 = the README chain) and in
every round, interleaved: the new call (one launch per RNVP layer), the same call from a
second trainer with one launch per net (DF_SCORE_PER_NET=1), df_train_gradient and the
inverse pass alone (df_chain_logpdf; it keeps no layer outputs, so it is a lower bound of the
inverse pass inside the two calls).  Every call is timed with device events after a
warm-up and bench.py's settle policy (untimed rounds until 0.3 s have passed).  Prints one
JSON line per config: median ms per call and Msamples/s, the sweep parts (call minus
inverse pass), and the effective shader clock of the inverse pass (df_chain_clock_probe).

--plain: no clock probe and no settle (for a profiler run: a few calls of each, nothing else).
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
    ap.add_argument("--configs", default="cfg2,cfg1")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--settle-seconds", type=float, default=0.3)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import bench
    from densityflows_amd import _lib
    from densityflows_amd.hip import _ptr, _stream
    from densityflows_amd.train import Adam, HIPTrainer

    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    B = args.batch
    for cfg in args.configs.split(","):
        chain = bench.build_chain(cfg)
        h = chain.hip()
        tr = HIPTrainer(h, Adam())
        tr.set_theta_input(_lib.DF_THETA_GIVEN)
        # the same call with one launch per net instead of one per RNVP layer (A/B; the
        # library reads DF_SCORE_PER_NET when a trainer is created)
        os.environ["DF_SCORE_PER_NET"] = "1"
        tr_net = HIPTrainer(h, Adam())
        tr_net.set_theta_input(_lib.DF_THETA_GIVEN)
        del os.environ["DF_SCORE_PER_NET"]
        d, n = h.d, h.n
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(B * d, generator=g, device=dev, dtype=torch.float32)
        th = torch.rand(B * n, generator=g, device=dev, dtype=torch.float32) if n else None
        lp = torch.empty(B, dtype=torch.float32, device=dev)
        gx = torch.empty(B * d, dtype=torch.float32, device=dev)
        gth = torch.empty(B * n, dtype=torch.float32, device=dev) if n else None
        lpsum = torch.zeros(1, dtype=torch.float64, device=dev)

        def inverse():
            _lib.check(h.lib.df_chain_logpdf(h.handle, _ptr(x), _ptr(th), _ptr(lp), C.c_int64(B), _stream(dev)))

        legs = {"logpdf_grad": lambda: tr.logpdf_grad(x, th, B, lp, gx, gth),
                "logpdf_grad_per_net": lambda: tr_net.logpdf_grad(x, th, B, lp, gx, gth),
                "train_gradient": lambda: tr.gradient(x, th, B, B, lpsum),
                "inverse_pass": inverse}

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
        while not args.plain and time.perf_counter() - t_warm < args.settle_seconds and settle < 10000:
            round_()
            torch.cuda.synchronize()
            settle += 1
        times = {k: [] for k in legs}
        for _ in range(args.calls):
            round_(times)
        torch.cuda.synchronize()
        res = {"config": cfg, "batch": B, "d": d, "n": n, "calls": args.calls, "settle_rounds": settle,
               "interleaved": list(legs)}
        med = {}
        for name, evs in times.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            med[name] = statistics.median(ms)
            res[name] = {"ms_median": round(med[name], 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                         "msamples_per_s": round(B / med[name] / 1e3, 2)}
        res["sweep_ms"] = {"logpdf_grad": round(med["logpdf_grad"] - med["inverse_pass"], 4),
                           "logpdf_grad_per_net": round(med["logpdf_grad_per_net"] - med["inverse_pass"], 4),
                           "train_gradient": round(med["train_gradient"] - med["inverse_pass"], 4)}
        if not args.plain:
            h.clock_probe(True)
            for _ in range(5):
                inverse()
            torch.cuda.synchronize()
            ghz_med, ghz_mean, slots = h.clock_read()
            h.clock_probe(False)
            res["inverse_pass_clock_ghz"] = {"median": round(ghz_med, 4), "mean": round(ghz_mean, 4), "slots": slots}
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        tr.close()
        tr_net.close()


if __name__ == "__main__":
    main()
