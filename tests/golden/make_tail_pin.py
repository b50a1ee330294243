"""Pinned bits of the specialised SPLIT kernel on models that reach every path of its
net-body tail (tests/test_gpu_split_tail.py).

The tail of a net body in densityflows.jl_amd/csrc/df_uniform_impl.h (the transposed
reduction of the output GEMV, the coupling, the ldj update of the state rows) and the
first-Dense split in front of it may be re-arranged as long as every sum keeps its
association and every rounding its place: the outputs are pinned bit for bit.  This
generator needs an MI355X and the built library; it wrote the committed ``tail_pin_*.npz``
on commit

    e941aee  (Sample weights on the device: weighted NLL, gradients, steps, epochs)

that is, on the build BEFORE the tail was changed.  Regenerate only when a change is MEANT
to alter the arithmetic, and state the commit here (``--commit <sha>`` records it in
tail_pin_meta.json).

Models (seeded; biases and output scale as bench._init_nets; each selects kernel id 4).  A
model is a list of flow elements; an element of several layers is a nested FlowChain, whose
layers share one ldj accumulator (first_in_elem / last_in_elem differ within it).  A net of
a d = 5 layer with one output has four conditioner inputs, one more than the specialised
kernel takes, so the one-output tails are reached at d = 4 and the four-output ones at d = 5.
  h64_d4 / h32_d4   d = 4: outputs 1 | (2, 1) | 3 | NICE 1 + RNVP 2 — an element of one RNVP
                    layer FIRST (have_acc false) and later (have_acc true), elements of
                    two, a NICE layer in the middle of the chain and first in its element
  h64_d5 / h32_d5   d = 5: NICE 2 first | (4, 2) | NormalizationLayer | 3 | (2, NICE 4) |
                    (3, 4) — a NICE layer first in the chain, one last in its element, a
                    NormalizationLayer between elements (an element of its own), masks
                    given unsorted
  h64_theta         d = 4, n = 1 with θ bounds, unsorted masks: 2 | (3, 4) | 2
Every net with 1..4 outputs so runs as an s- and as a t-phase, at hidden 64 and 32.

Tile settings (DF_TILES when the handle is created): 2 (one tile group per wave), 4 and the
plan's maximum (recorded in tail_pin_meta.json from the launch line of the generating
build; the test checks the launches against it).  Batches per setting, S = 128 · tiles:
1, 17, S - 1, S, S + 1, 2S + 33.

Per model and batch: forward x / ldj, inverse x / ldj, per-sample logpdf; forward! is not
stored, its x equals forward's bit for bit (asserted here and in the test).  A launch's
per-sample bits do not depend on the tile count, so those are kept per batch: in full for
batches up to FULL_MAX and as SHA-256 of the array's bytes above (the pin files stay the
size of the earlier ones).  The fp64 NLL partial sum adds per workgroup, so it is kept per
(tiles, batch).
"""
import hashlib
import json
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PARENT = "e941aee"
PASSES = ("fwd_x", "fwd_ldj", "inv_x", "inv_ldj", "logpdf")
FULL_MAX = 600
_D4 = [[("rnvp", [4])], [("rnvp", [2, 1]), ("rnvp", [3])], [("rnvp", [2, 3, 4])], [("nice", [1]), ("rnvp", [4, 2])]]
_D5 = [[("nice", [2, 1])], [("rnvp", [1, 2, 3, 4]), ("rnvp", [5, 3])], "norm", [("rnvp", [4, 5, 3])],
       [("rnvp", [2, 1]), ("nice", [5, 4, 3, 1])], [("rnvp", [3, 1, 2]), ("rnvp", [5, 2, 4, 3])]]
# name: (d, n, hidden, seed, elements); an element is a list of (kind, mask) or "norm";
# masks are the transformed dims (1-based)
MODELS = {
    "h64_d4": (4, 0, 64, 301, _D4),
    "h32_d4": (4, 0, 32, 302, _D4),
    "h64_d5": (5, 0, 64, 303, _D5),
    "h32_d5": (5, 0, 32, 304, _D5),
    "h64_theta": (4, 1, 64, 305, [[("rnvp", [4, 3])], [("rnvp", [3, 1, 2]), ("rnvp", [4, 2, 1, 3])], [("rnvp", [2, 1])]]),
}
NORM_BOUNDS = (np.array([-3.0, -2.5, -4.0, -3.5, -2.0], np.float32), np.array([3.5, 2.0, 3.0, 4.0, 2.5], np.float32))
THETA_BOUNDS = (np.array([-0.25], np.float32), np.array([1.5], np.float32))
LAUNCH = re.compile(r"\[df\] mode (\d+) batch (\d+) kernel (\S+) tiles (\d+) \(max (\d+)\)")


def samples_per_block(tiles):
    return 8 * 16 * tiles


def batches(tiles):
    S = samples_per_block(tiles)
    return (1, 17, S - 1, S, S + 1, 2 * S + 33)


def tile_settings(max_tiles):
    """The tiles per wave the launches are forced to (DF_TILES)."""
    return sorted({t for t in (2, 4, max_tiles) if t <= max_tiles})


def all_batches(max_tiles):
    return sorted({B for t in tile_settings(max_tiles) for B in batches(t)})


def path(name):
    return os.path.join(HERE, f"tail_pin_{name}.npz")


def meta():
    with open(os.path.join(HERE, "tail_pin_meta.json")) as f:
        return json.load(f)


def build_model(name):
    import bench
    import densityflows_amd as dfa

    d, n, hidden, seed, elements = MODELS[name]
    rng = np.random.default_rng(seed)
    kinds = {"rnvp": dfa.RNVPCouplingLayer, "nice": dfa.NICECouplingLayer}
    els, flat = [], []
    for e in elements:
        if e == "norm":
            els.append(dfa.NormalizationLayer(NORM_BOUNDS[0], NORM_BOUNDS[1], -1.0, 1.0))
            continue
        ls = [dfa.CouplingLayer(kinds[k], d, m, n=n, hidden_dim=hidden, rng=rng) for k, m in e]
        flat += ls
        els.append(ls[0] if len(ls) == 1 else dfa.FlowChain(*ls))
    bench._init_nets(dfa.FlowChain(*flat), rng)
    return dfa.FlowChain(*els)


def compile_model(name):
    """A fresh handle (the plan reads DF_TILES when it is created)."""
    n = MODELS[name][1]
    hc = build_model(name).hip(device=0, n_hint=n)
    assert hc.info.kernel == 4, (name, hc.info.kernel)  # the specialised SPLIT kernel
    if n:
        hc.set_theta_bounds(*THETA_BOUNDS)
    return hc


def inputs(name, B):
    """z, the inverse / logpdf input x and θ, flat and sample-major."""
    d, n, _, seed, _ = MODELS[name]
    rng = np.random.default_rng(1000 * seed + B)
    z = rng.standard_normal((B, d)).astype(np.float32).reshape(-1)
    x = rng.standard_normal((B, d)).astype(np.float32).reshape(-1)
    th = (rng.random((B, n)) * 1.5 - 0.2).astype(np.float32).reshape(-1) if n else None
    return z, x, th


def passes(hc, name, B):
    """The pinned arrays of one model at one batch size, forward!'s x (fwdi_x) and the
    fp64 NLL partial sum (nll, one float64) beside them."""
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
    s = torch.zeros(1, dtype=torch.float64, device=dev)
    hc.run_logpdf_sum(tx, tth, s, B)
    torch.cuda.synchronize()
    got = dict(zip(PASSES, (x, ldj, zb, ldjb, lp)))
    got["fwdi_x"], got["nll"] = zi, s
    return {k: v.cpu().numpy() for k, v in got.items()}


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def pinned(a, B):
    """What the pin file holds for array a of batch B: the array, or its SHA-256."""
    return a if B <= FULL_MAX else digest(a)


def launch_lines(fn):
    """Run fn() with the process's stderr in a file; its result and the launch lines."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            sys.stderr.flush()
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        text = f.read().decode(errors="replace")
    return out, LAUNCH.findall(text)


def main():
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unstated"
    assert commit.startswith(PARENT), f"the pins come from a build of {PARENT}, not {commit}"
    total, max_tiles = 0, {}
    os.environ["DF_DEBUG_LAUNCH"] = "1"
    for name in MODELS:
        os.environ["DF_TILES"] = "2"
        hc = compile_model(name)
        _, ran = launch_lines(lambda: passes(hc, name, 17))
        assert ran and all(k == "uniform-fast-split" and int(t) == 2 for _, _, k, t, _ in ran), ran
        mt = max_tiles[name] = int(ran[0][4])
        out, seen = {}, set()
        for tiles in tile_settings(mt):
            os.environ["DF_TILES"] = str(tiles)
            hc = compile_model(name)
            for B in batches(tiles):
                got, ran = launch_lines(lambda: passes(hc, name, B))
                assert ran and all(int(t) == tiles for _, _, _, t, _ in ran), (name, tiles, B, ran)
                again = passes(hc, name, B)
                for k in got:
                    assert np.array_equal(again[k].view(np.uint8), got[k].view(np.uint8)), (name, k, B)
                    assert np.all(np.isfinite(got[k])), (name, k, B)
                assert np.array_equal(got["fwdi_x"].view(np.uint32), got["fwd_x"].view(np.uint32)), (name, B)
                out[f"nll_t{tiles}_{B}"] = got["nll"]
                for k in PASSES:
                    p = pinned(got[k], B)
                    if B in seen:  # the per-sample bits do not depend on the tile count
                        assert np.array_equal(out[f"{k}_{B}"].view(np.uint8), p.view(np.uint8)), (name, k, B, tiles)
                    out[f"{k}_{B}"] = p
                seen.add(B)
        np.savez(path(name), **out)
        total += os.path.getsize(path(name))
    with open(os.path.join(HERE, "tail_pin_meta.json"), "w") as f:
        json.dump({"commit": commit, "models": sorted(MODELS), "max_tiles": max_tiles, "full_max": FULL_MAX}, f, indent=1)
        f.write("\n")
    print("wrote", len(MODELS), "models,", total, "bytes, commit", commit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
