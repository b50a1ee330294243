"""Timing of truncated sampling (df_flow_sample_region) beside its two alternatives.

    python tools/reject_ab.py [--config cfg1 cfg2] [--n-want 1048576] [--reps 20] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/reject_ab.py --config cfg2 --profile

bench.py's README chain (cfg1) and config-2 chain, a box with acceptance near one half
(quantiles of a seeded sample), n_want accepted samples.  Three arms, one process, interleaved
repetition by repetition after a warm-up and 0.3 s of untimed repetitions; each arm ends in a
device synchronise and is timed with the host clock; median and range are reported:

  (a) region   sample_with_rejection's device path, adaptive rounds: one library call
  (b) sample   df_flow_sample of as many candidates as (a) drew in whole rounds, in one call:
               the cost with no filtering at all
  (c) host     the closure path's data movement with the per-candidate Python call replaced
               by ONE vectorised numpy box test per round (a stand-in: the real closure path
               calls Python once per candidate, which dominates everything else): per round
               df_flow_sample, device→host copy of the candidates, numpy filter, host→device
               copy of the kept rows

(a) and (c) must return bitwise the same samples and counts.  --profile runs one (a) call
only, for a kernel trace taken in a run of its own.  Prints one JSON line per config.
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

SEED = 5
THETA = {"cfg1": (0.3,), "cfg2": ()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["cfg1", "cfg2"], choices=["cfg1", "cfg2"])
    ap.add_argument("--n-want", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle-seconds", type=float, default=0.3)
    ap.add_argument("--profile", action="store_true", help="one region call per config and nothing else")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch

    import bench
    import densityflows_amd as dfa
    from densityflows_amd import flows

    if not torch.cuda.is_available():
        raise SystemExit("reject_ab needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)
    n_want = args.n_want
    max_tries = 100 * n_want

    for config in args.config:
        d, n, _ = bench.CONFIGS[config]
        flow = dfa.Flow(bench.build_chain(config),
                        metadata=dfa.MetaData("", d, n, np.zeros(n, np.float32), np.ones(n, np.float32)))
        h = flow.hip(device=0)
        theta = THETA[config]
        thvec = torch.tensor(theta, dtype=torch.float32, device=dev) if n else None
        x = dfa.sample(flow, 4096, theta if n else None, seed=11).cpu().numpy()
        lo = np.quantile(x, 0.07, axis=1).astype(np.float32)
        hi = np.quantile(x, 0.93, axis=1).astype(np.float32)
        lo[-1] = -np.inf
        region = dfa.Region(dfa.Box(lo, hi)).arrays(d)
        out_a = torch.empty(d * n_want, dtype=torch.float32, device=dev)
        out_c = torch.empty(d * n_want, dtype=torch.float32, device=dev)

        def arm_region():
            return h.run_sample_region(out_a, thvec, n_want, *region, max_tries, 0, SEED)

        if args.profile:
            tried, accepted = arm_region()
            torch.cuda.synchronize()
            print(json.dumps({"config": config, "profile_call": True, "tried": tried, "accepted": accepted}), flush=True)
            continue

        rounds = []

        def arm_host(record=False):
            """The closure path's schedule and copies, the predicate vectorised."""
            R = flows._first_round(n_want)
            k0 = accepted = 0
            rows_out = out_c.view(-1, d)
            while k0 < max_tries:
                cand = torch.empty(R * d, dtype=torch.float32, device=dev)
                h.run_sample(cand, thvec, n > 0, R, SEED, d * (k0 // 4))
                rows = cand.cpu().numpy().reshape(R, d)
                if record:
                    rounds.append(R)
                count = min(R, max_tries - k0)
                keep = np.flatnonzero(np.all((lo <= rows[:count]) & (rows[:count] <= hi), axis=1))[:n_want - accepted]
                rows_out[accepted:accepted + len(keep)].copy_(torch.from_numpy(rows[keep]).to(dev))
                accepted += len(keep)
                if accepted == n_want:
                    torch.cuda.synchronize()
                    return k0 + int(keep[-1]) + 1, accepted
                k0 += count
                R = flows._next_round(n_want - accepted, k0, accepted, R)
            raise SystemExit("the box was never filled")

        counts_c = arm_host(record=True)
        drawn = sum(rounds)
        cand_b = torch.empty(drawn * d, dtype=torch.float32, device=dev)

        def arm_sample():
            h.run_sample(cand_b, thvec, n > 0, drawn, SEED, 0)
            torch.cuda.synchronize()

        arms = {"region": arm_region, "sample": arm_sample, "host": arm_host}
        for f in arms.values():
            for _ in range(3):
                f()
        counts_a = arm_region()
        torch.cuda.synchronize()
        same = counts_a == counts_c and bool(torch.equal(out_a.view(torch.int32), out_c.view(torch.int32)))
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.settle_seconds:
            for f in arms.values():
                f()

        ms = {name: [] for name in arms}
        for _ in range(args.reps):
            for name, f in arms.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t) * 1e3)
        stat = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                       "max_ms": round(max(v), 4)} for name, v in ms.items()}
        med = {name: s["median_ms"] for name, s in stat.items()}
        line = {"config": config, "d": d, "n": n, "n_want": n_want, "tried": counts_a[0], "accepted": counts_a[1],
                "acceptance": round(counts_a[1] / counts_a[0], 4), "rounds": rounds, "candidates_drawn": drawn,
                "reps": args.reps, "region_equals_host_bitwise": same, "arms": stat,
                "region_over_sample": round(med["region"] / med["sample"], 4),
                "region_over_host": round(med["region"] / med["host"], 4),
                "host_arm": "vectorised numpy predicate (stand-in for the per-candidate closure)"}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
        if not same:
            raise SystemExit("region and host paths differ")


if __name__ == "__main__":
    main()
