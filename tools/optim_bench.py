"""Timing of the optimiser chains.

    python tools/optim_bench.py [--rounds 5] [--out FILE]

Two measurements on one build, device events around runs of calls, after a warm-up:
  * df_train_apply at config 5's parameter count (2,441,728 parameters in 192 tensors) with a
    fixed gradient in the buffer, for the plain Adam trainer, [Adam, WeightDecay] (the fused
    chain kernel in place of adam_kernel) and [ClipNorm, Adam, WeightDecay] (plus the
    per-tensor Σ dx² kernel);
  * the README chain (hidden 16, 2,322 parameters) through df_train_step_graph at batch 64,
    where the step is launch-bound and replayed as one hipGraph, for the same three: the cost
    of the chain kernel and of the extra graph node.
Prints one JSON line (µs per call: every round, and the median).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()

    import torch

    import densityflows_amd  # noqa: F401  (the package: the symlink at the repository root)
    from densityflows_amd.train import Adam, ClipNorm, HIPTrainer, OptimiserChain, WeightDecay
    from helpers import spec_to_element
    from oracle import flow_oracle as O

    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs an MI355X: no HIP device visible")
    dev = torch.device("cuda", 0)

    def timed(fn, warm, reps):
        for _ in range(warm):
            fn()
        out = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(round(a.elapsed_time(b) * 1e3 / reps, 2))
        return {"us": out, "median_us": statistics.median(out)}

    opts = [("Adam", lambda w: Adam(1e-3)),
            ("[Adam, WeightDecay]", lambda w: OptimiserChain(Adam(1e-3), WeightDecay(1e-3))),
            ("[ClipNorm, Adam, WeightDecay]", lambda w: OptimiserChain(ClipNorm(w), Adam(1e-3), WeightDecay(1e-3)))]
    res = {"apply_cfg5": {}, "readme_step_graph_b64": {}}

    rng = np.random.default_rng(0)
    spec5 = {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(32, n=8), hidden=256, bias_scale=0.1, out_scale=0.1)
        for _ in range(8)]}
    for label, mk in opts:
        tr = HIPTrainer(spec_to_element(spec5).hip(), mk(0.01))
        g = (np.random.default_rng(1).standard_normal(tr.num_params) * 1e-3).astype(np.float32)
        tr.grad().copy_(torch.from_numpy(g))
        res["apply_cfg5"][label] = timed(tr.apply, 20, 100)
        res["n_params_cfg5"], res["n_tensors_cfg5"] = tr.num_params, int(tr.tensor_offsets().shape[0] - 1)
        del tr

    rng = np.random.default_rng(0)
    layers = [O.rnvp_layer(rng, O.coupling_axes(5, m, n=1), hidden=16, bias_scale=0.1, out_scale=0.5)
              for m in ([1, 2, 3], [3, 4, 5], [5, 1, 2])]
    layers.append({"kind": "norm", "x_min": np.full(5, -3.0, np.float32), "x_max": np.full(5, 2.5, np.float32),
                   "alpha": -1.0, "beta": 1.0})
    spec = {"kind": "chain", "layers": layers}
    x = torch.from_numpy(rng.standard_normal((64, 5)).astype(np.float32).ravel()).to(dev)
    th = torch.from_numpy(rng.random((64, 1)).astype(np.float32).ravel()).to(dev)
    for label, mk in opts:
        tr = HIPTrainer(spec_to_element(spec).hip(), mk(0.5))
        res["readme_step_graph_b64"][label] = timed(lambda: tr.step_graph(x, th, 64), 50, 1000)
        del tr

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
