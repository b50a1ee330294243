"""Pinned bits of the specialised SPLIT kernel on models that reach every path of its
net-body head (tests/test_gpu_split_head.py).

The head of a net body in densityflows.jl_amd/csrc/df_uniform_impl.h (the per-layer slot
words, the stage offsets, the first-Dense fragments, the features and step 0 of the hidden
Dense) and the wave priorities of its phases move loads, waits, scalar registers and issue
order only: the arithmetic, its order and every rounding stay, so the outputs are pinned
bit for bit.  This generator needs an MI355X and the built library; it wrote the committed
``head_pin_*.npz`` on commit

    68d92c8  (Batch-edge and tiles-per-wave tests for every chain-pass kernel)

that is, on the build BEFORE the head was changed.  Regenerate only when a change is MEANT
to alter the arithmetic, and state the commit here (``--commit <sha>`` records it in
head_pin_meta.json).

Models (seeded; biases and output scale as bench._init_nets; each selects kernel id 4):
  h32_ten_nets            d = 5, five RNVP layers, hidden 32.  The split blob is past
                          64 KiB, so 24 KiB stages of two nets each: net offsets != 0, and
                          the second net of a stage finds it resident (ensure_stage returns
                          early; the schedule position must not advance).  Every net of
                          hidden 32 is 8.3-8.7 KiB, so a stage always holds the s- and
                          t-net of ONE layer: its switches fall between layers.
  h32_nice_shift          as h32_ten_nets behind a leading NICE layer (one net), which
                          shifts the pairing: every stage holds the t-net of one layer and
                          the s-net of the next, so the switches fall BETWEEN the s- and
                          t-net of a layer, in both pass directions, and consecutive nets
                          of the same stage belong to different layers (different slot
                          words on the same stage offsets).
  h64_theta_unsorted_norm d = 5, n = 1, unsorted masks with 3 transformed dims, a
                          NormalizationLayer between the coupling layers, θ bounds set: the
                          conditioner input is θ and two z dims (all three feature slots
                          beside the bias slot), slot words that mix θ and z columns, a
                          NORM layer between two descriptor loads and a last net without a
                          successor.  Hidden 64: every net is a stage of its own, so every
                          net starts behind a switch.
  h64_nice_first          d = 5, NICE first and last (one net per layer at both ends of
                          either pass), RNVP between.

Tile settings (DF_TILES when the handle is created): unset and 2 — at these batch sizes
both run one two-tile group per wave (the launcher takes the fewest tiles that fill one
round), S = 256 samples per workgroup — and 4 where the plan holds 4 resident tiles
(MAX_TILES below, checked against the planner by tests/test_split_head_words.py): two tile
groups per net, S = 512.  Batches per setting: 1, 17, S - 1, S + 1, 2S + 33.  A launch's
bits do not depend on the tile count, so the pins are kept per batch.

Per model and batch: forward x / ldj, inverse x / ldj, per-sample logpdf.  forward! is not
stored: its x equals forward's bit for bit (asserted here on the generating build and in
the test against the forward pin).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import make_prefetch_pin as PF  # noqa: E402  (inputs' layout, the six passes)

PARENT = "68d92c8"
PASSES = ("fwd_x", "fwd_ldj", "inv_x", "inv_ldj", "logpdf")
# name: (d, n, hidden, seed, [(kind, mask), ...]); masks are the transformed dims (1-based)
MODELS = {
    "h32_ten_nets": (5, 0, 32, 201, [("rnvp", [1, 2, 3]), ("rnvp", [4, 5]), ("rnvp", [2, 3, 4, 5]),
                                     ("rnvp", [1, 5, 3]), ("rnvp", [4, 2])]),
    "h32_nice_shift": (5, 0, 32, 202, [("nice", [4, 5]), ("rnvp", [1, 2, 3]), ("rnvp", [5, 4]),
                                       ("rnvp", [3, 1, 2]), ("rnvp", [2, 5, 4, 3]), ("rnvp", [1, 4])]),
    "h64_theta_unsorted_norm": (5, 1, 64, 203, [("rnvp", [4, 1, 3]), ("norm", None), ("rnvp", [5, 2, 4])]),
    "h64_nice_first": (5, 0, 64, 204, [("nice", [3, 1]), ("rnvp", [2, 4, 5]), ("rnvp", [5, 1, 3]),
                                       ("nice", [4, 2, 1])]),
}
# resident 16-sample tiles per wave of the SPLIT plan (df::Plan::stiles)
MAX_TILES = {"h32_ten_nets": 8, "h32_nice_shift": 8, "h64_theta_unsorted_norm": 2, "h64_nice_first": 4}
NORM_BOUNDS = (np.array([-3.0, -2.5, -4.0, -3.5, -2.0], np.float32), np.array([3.5, 2.0, 3.0, 4.0, 2.5], np.float32))
THETA_BOUNDS = (np.array([-0.25], np.float32), np.array([1.5], np.float32))


def samples_per_block(tiles):
    return 8 * 16 * tiles


def tile_settings(name):
    """(DF_TILES value or None, tiles per wave the launches run)."""
    out = [(None, 2), ("2", 2)]
    if MAX_TILES[name] >= 4:
        out.append(("4", 4))
    return out


def batches(tiles):
    S = samples_per_block(tiles)
    return (1, 17, S - 1, S + 1, 2 * S + 33)


def all_batches(name):
    return sorted({B for _, t in tile_settings(name) for B in batches(t)})


def path(name):
    return os.path.join(HERE, f"head_pin_{name}.npz")


def build_model(name):
    import bench
    import densityflows_amd as dfa

    d, n, hidden, seed, layers = MODELS[name]
    rng = np.random.default_rng(seed)
    kinds = {"rnvp": dfa.RNVPCouplingLayer, "nice": dfa.NICECouplingLayer}
    els = []
    for k, m in layers:
        if k == "norm":
            els.append(dfa.NormalizationLayer(NORM_BOUNDS[0], NORM_BOUNDS[1], -1.0, 1.0))
        else:
            els.append(dfa.CouplingLayer(kinds[k], d, m, n=n, hidden_dim=hidden, rng=rng))
    return bench._init_nets(dfa.FlowChain(*els), rng)


def compile_model(name):
    """A fresh handle (the plan reads DF_TILES when it is created)."""
    n = MODELS[name][1]
    hc = build_model(name).hip(device=0, n_hint=n)
    assert hc.info.kernel == 4, (name, hc.info.kernel)  # the specialised SPLIT kernel
    if n:
        hc.set_theta_bounds(*THETA_BOUNDS)
    return hc


def passes(hc, name, B):
    """The pinned arrays of one model at one batch size, and forward!'s x beside them."""
    PF.MODELS[name] = MODELS[name]  # PF.inputs reads (d, n, seed) of the model
    try:
        got = PF.passes(hc, name, B)
    finally:
        del PF.MODELS[name]
    return got


def main():
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unstated"
    assert commit.startswith(PARENT), f"the pins come from a build of {PARENT}, not {commit}"
    total = 0
    for name in MODELS:
        os.environ.pop("DF_TILES", None)
        hc = compile_model(name)
        out = {}
        for B in all_batches(name):
            got = passes(hc, name, B)
            assert np.array_equal(got["fwdi_x"].view(np.uint32), got["fwd_x"].view(np.uint32)), (name, B)
            for k in PASSES:
                assert np.all(np.isfinite(got[k])), (name, k, B)
                out[f"{k}_{B}"] = got[k]
        np.savez(path(name), **out)
        total += os.path.getsize(path(name))
    with open(os.path.join(HERE, "head_pin_meta.json"), "w") as f:
        json.dump({"commit": commit, "models": sorted(MODELS), "max_tiles": MAX_TILES}, f, indent=1)
        f.write("\n")
    print("wrote", len(MODELS), "models,", total, "bytes, commit", commit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
