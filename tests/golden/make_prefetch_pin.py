"""Pinned bits of the specialised SPLIT kernel on small models that reach every path of
its LDS-read placement (tests/test_gpu_split_prefetch.py).

The fragment prefetch of the hidden Dense, the batched first-Dense reads and the batched
tail reads of densityflows.jl_amd/csrc/df_uniform_impl.h move LDS reads and waits only:
the arithmetic, its order and every rounding stay, so the outputs are pinned bit for bit.
This generator needs an MI355X and the built library; it wrote the committed
``prefetch_pin_*.npz`` on commit

    98ed9fa  (Add df_train_logpdf_grad: per-sample ∂logpdf/∂x and ∂logpdf/∂θ on device)

that is, on the build BEFORE any read was moved.  Regenerate only when a change is MEANT
to alter the arithmetic, and state the commit here (``--commit <sha>`` records it in
prefetch_pin_meta.json).

Models (seeded; biases and output scale as bench._init_nets; each selects kernel id 4):
  h64_d5     hidden 64 (HT = 4, two k-chunks), d = 5: RNVP layers with 4, 3, 2, 4, 2 outputs
  h64_d4     hidden 64, d = 4: RNVP layers with 1, 3, 1, 2 outputs
  h32_d5     hidden 32 (HT = 2: one chunk, no chunk boundary in the pipeline), as h64_d5
  h32_d4     hidden 32, as h64_d4
  h64_theta  hidden 64, d = 4, n = 1 (θ): 2, 3, 2 outputs
  h64_nice   hidden 64, d = 5: RNVP (3), NICE (2), RNVP (4), NICE (3)
A net with one output of a d = 5 layer has four conditioner inputs, one more than the
specialised kernel's single folded first-Dense k-step takes (the planner then selects
another kernel), so the one-output tails are reached at d = 4.

Batch sizes 1, 17, 32, 33, 48, 511, 513: a partial tile, exactly one two-tile group, a
group plus a remainder, and a partial workgroup either side of 512.  Per model and batch:
forward x / ldj, forward! x, inverse x / ldj and per-sample logpdf.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCHES = (1, 17, 32, 33, 48, 511, 513)
PASSES = ("fwd_x", "fwd_ldj", "fwdi_x", "inv_x", "inv_ldj", "logpdf")
# name: (d, n, hidden, seed, [(kind, mask), ...]); masks are the transformed dims (1-based)
MODELS = {
    "h64_d5": (5, 0, 64, 101, [("rnvp", [1, 2, 3, 4]), ("rnvp", [3, 4, 5]), ("rnvp", [1, 2]),
                               ("rnvp", [5, 4, 3, 2]), ("rnvp", [2, 4])]),
    "h64_d4": (4, 0, 64, 102, [("rnvp", [4]), ("rnvp", [1, 2, 3]), ("rnvp", [2]), ("rnvp", [1, 3])]),
    "h32_d5": (5, 0, 32, 103, [("rnvp", [1, 2, 3, 4]), ("rnvp", [3, 4, 5]), ("rnvp", [1, 2]),
                               ("rnvp", [5, 4, 3, 2]), ("rnvp", [2, 4])]),
    "h32_d4": (4, 0, 32, 104, [("rnvp", [4]), ("rnvp", [1, 2, 3]), ("rnvp", [2]), ("rnvp", [1, 3])]),
    "h64_theta": (4, 1, 64, 105, [("rnvp", [3, 4]), ("rnvp", [1, 2, 3]), ("rnvp", [1, 2])]),
    "h64_nice": (5, 0, 64, 106, [("rnvp", [1, 2, 3]), ("nice", [4, 5]), ("rnvp", [2, 3, 4, 5]),
                                 ("nice", [1, 2, 3])]),
}


def path(name):
    return os.path.join(HERE, f"prefetch_pin_{name}.npz")


def build_model(name):
    import bench
    import densityflows_amd as dfa

    d, n, hidden, seed, layers = MODELS[name]
    rng = np.random.default_rng(seed)
    kinds = {"rnvp": dfa.RNVPCouplingLayer, "nice": dfa.NICECouplingLayer}
    ch = dfa.FlowChain(*[dfa.CouplingLayer(kinds[k], d, m, n=n, hidden_dim=hidden, rng=rng) for k, m in layers])
    return bench._init_nets(ch, rng)


def inputs(name, B):
    """z, the inverse / logpdf input x and θ, flat and sample-major (Julia's (d, B) column-major)."""
    d, n, _, seed, _ = MODELS[name]
    rng = np.random.default_rng(1000 * seed + B)
    z = rng.standard_normal((B, d)).astype(np.float32).reshape(-1)
    x = rng.standard_normal((B, d)).astype(np.float32).reshape(-1)
    th = rng.random((B, n)).astype(np.float32).reshape(-1) if n else None
    return z, x, th


def compile_model(name):
    n = MODELS[name][1]
    hc = build_model(name).hip(device=0, n_hint=n)
    assert hc.info.kernel == 4, (name, hc.info.kernel)  # the specialised SPLIT kernel
    if n:  # the logpdf pass normalises θ: bounds (0, 1) leave it as drawn
        hc.set_theta_bounds(np.zeros(n, np.float32), np.ones(n, np.float32))
    return hc


def passes(hc, name, B):
    """The six pinned arrays of one model at one batch size, from the loaded library."""
    import torch

    dev = torch.device("cuda", 0)
    z, xin, th = inputs(name, B)
    tz, tx = torch.from_numpy(z).to(dev), torch.from_numpy(xin).to(dev)
    tth = torch.from_numpy(th).to(dev) if th is not None else None
    x, ldj = torch.empty_like(tz), torch.empty(B, device=dev)
    hc.run("forward", tz, tth, x, ldj, B)
    zi = tz.clone()
    hc.run_inplace(zi, tth, B)
    zb, ldjb, lp = torch.empty_like(tx), torch.empty(B, device=dev), torch.empty(B, device=dev)
    hc.run("backward", tx, tth, zb, ldjb, B)
    hc.run_logpdf(tx, tth, lp, B)
    torch.cuda.synchronize()
    got = (x, ldj, zi, zb, ldjb, lp)
    return {k: v.cpu().numpy() for k, v in zip(PASSES, got)}


def compute(name):
    hc = compile_model(name)
    return {f"{k}_{B}": v for B in BATCHES for k, v in passes(hc, name, B).items()}


def main():
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unstated"
    total = 0
    for name in MODELS:
        out = compute(name)
        for k, v in out.items():
            assert np.all(np.isfinite(v)), (name, k)
        np.savez(path(name), **out)
        total += os.path.getsize(path(name))
    with open(os.path.join(HERE, "prefetch_pin_meta.json"), "w") as f:
        json.dump({"commit": commit, "batches": list(BATCHES), "models": sorted(MODELS)}, f, indent=1)
        f.write("\n")
    print("wrote", len(MODELS), "models,", total, "bytes, commit", commit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
