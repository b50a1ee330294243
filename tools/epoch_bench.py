"""Wall-clock cost of one train_ epoch with the host loader and with the device loader
(DESIGN §3.3, §4).

    timeout 600 python tools/epoch_bench.py [--epochs 3] [--n 64000] [--out FILE]

The README chain (hidden 16, 2,322 parameters) on a synthetic set of --n training samples
(and --n / 10 validation samples), shuffle on, at batchsize 64 (1000 steps per epoch at the
default --n) and at batchsize 4096.  Per batchsize: two flows from the same weights, one per
loader; one warm-up epoch each, then --epochs timed epochs each, alternating host / device.
An epoch is one train_(epochs=1) call, so it holds what a user's epoch holds: the
mini-batch steps, the two epoch losses and the read-back (train_ ends on a device
synchronise); for the device loader also the upload of both sets, which a longer run pays
once.  After them HIPTrainer.epoch alone on buffers that stay (the resident loop without
losses or uploads), and the effective shader clock of one pass over the set.
Prints one JSON line: ms per epoch of every timed epoch, the median, and µs per step.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--n", type=int, default=64000, help="training samples")
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()

    import torch

    import densityflows_amd as dfa
    from densityflows_amd.train import Adam, setup, train_, trainables

    if not torch.cuda.is_available():
        raise SystemExit("epoch_bench needs an MI355X: no HIP device visible")

    n_valid = args.n // 10
    total = args.n + n_valid

    def make():
        rng = np.random.default_rng(0)
        x = rng.standard_normal((5, total)).astype(np.float32)
        th = rng.random((1, total)).astype(np.float32)
        data = dfa.DataArrays(x, th, f_training=args.n / total, f_validation=n_valid / total, rng=rng)
        chain = dfa.FlowChain(
            dfa.CouplingLayer(data, [1, 2, 3], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
            dfa.CouplingLayer(data, [3, 4, 5], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
            dfa.CouplingLayer(data, [5, 1, 2], hidden_dim_s=16, hidden_dim_t=16, rng=rng),
            dfa.NormalizationLayer.from_data(x, -1.0, 1.0))
        flow = dfa.Flow(chain, data)
        assert data.training_data()[0].shape[1] == args.n
        return data, chain, flow, setup(Adam(1e-3), flow)

    res = {"n_train": args.n, "n_valid": n_valid, "epochs": args.epochs}
    for bs in (64, 4096):
        steps = -(-args.n // bs)
        runs = {ld: make() + (np.random.default_rng(1),) for ld in ("host", "device")}
        times = {"host": [], "device": []}

        def epoch(ld):
            data, chain, flow, state, rng = runs[ld]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_(flow, data, state, epochs=1, batchsize=bs, shuffle=True, verbose=False, rng=rng, loader=ld)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for ld in ("host", "device"):
            epoch(ld)  # warm-up: allocations, graph captures
        for _ in range(args.epochs):
            for ld in ("host", "device"):
                times[ld].append(round(epoch(ld), 3))
        # both loaders took the same steps from the same permutations
        same = bool(np.array_equal(trainables(runs["host"][1]), trainables(runs["device"][1])))
        out = {"steps_per_epoch": steps, "same_parameters": same}
        for ld in ("host", "device"):
            med = statistics.median(times[ld])
            out[ld] = {"ms_per_epoch": times[ld], "median_ms": round(med, 3),
                       "spread_ms": round(max(times[ld]) - min(times[ld]), 3),
                       "us_per_step": round(med * 1e3 / steps, 2)}
        out["host_over_device"] = round(out["host"]["median_ms"] / out["device"]["median_ms"], 3)
        # the resident loop alone (HIPTrainer.epoch on buffers that stay: no losses, no upload)
        data, chain, flow, state, rng = runs["device"]
        x_tr, th_tr = data.training_data()
        dev = state.trainer.device
        xs = torch.from_numpy(np.ascontiguousarray(x_tr.T).ravel()).to(dev)
        ts = torch.from_numpy(np.ascontiguousarray(th_tr.T).ravel()).to(dev)
        od = torch.from_numpy(rng.permutation(args.n).astype(np.int32)).to(dev)
        alone = []
        for i in range(args.epochs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            state.trainer.epoch(xs, ts, args.n, od, bs)
            torch.cuda.synchronize()
            alone.append(round((time.perf_counter() - t0) * 1e3, 3))
        med = statistics.median(alone[1:])
        out["epoch_call_alone"] = {"ms_per_epoch": alone[1:], "median_ms": round(med, 3),
                                   "us_per_step": round(med * 1e3 / steps, 2)}
        res[f"batchsize_{bs}"] = out

    # the box's effective shader clock, stamped by the chain-pass kernels of one pass over the set
    data, chain, flow, state, rng = runs["host"]
    h = flow.hip()
    h.clock_probe(True)
    h.logpdf_sum(*data.training_data())
    ghz_median, ghz_mean, slots = h.clock_read()
    h.clock_probe(False)
    res["shader_clock_ghz"] = {"median": round(ghz_median, 3), "mean": round(ghz_mean, 3), "slots": slots}

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
