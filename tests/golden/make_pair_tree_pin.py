"""Pinned bits of the specialised SPLIT kernel on models whose nets have three and four
outputs (tests/test_gpu_split_pair_tree.py), the companion of make_tail_pin.py.

The tail of a net body in densityflows.jl_amd/csrc/df_uniform_impl.h reduces the output
GEMV of BOTH tiles of a tile group in one pair of trees when the net has three or four
outputs, sums the s outputs of both tiles in one tree and updates both rows' ldj words
once.  Every sum keeps its association and every rounding its place, so the outputs are
pinned bit for bit.  This generator needs an MI355X and the built library; it wrote the
committed ``pair_tree_pin_*.npz`` on commit

    399df44  (Posterior histograms on the device: 1-D and 2-D marginal counts)

that is, on the build BEFORE the pair trees.  Regenerate only when a change is MEANT to
alter the arithmetic, and state the commit here (``--commit <sha>`` records it in
pair_tree_pin_meta.json).

Models (seeded; biases and output scale as bench._init_nets), each at hidden 64 and 32.  A
model is a list of flow elements; an element of several layers is a nested FlowChain, whose
layers share one ldj accumulator.  The specialised kernel takes a net of at most three
conditioner inputs, d - outputs of them at n = 0, so it runs d = 5 with 2..4 outputs, d = 6
with 3 and d = 7 with 4 outputs; a d = 7 layer of three outputs and every d = 8 layer have
four inputs and put their whole chain on another kernel.  Those two chains are pinned all
the same (the kernel they select is recorded and checked), and d6 / d7q reach the three-
and four-output bodies from both sides instead:
  d5      d = 5: 2 | 3 | 2 | 3, masks as in a CouplingBlock chain, one layer per element
  d7      d = 7: 3 | 4 (a CouplingBlock's masks)            — not the specialised kernel
  d8      d = 8: 4 | 4 (a CouplingBlock's masks)            — not the specialised kernel
  d6      d = 6: 3 | 3 | 3
  d7q     d = 7: 4 | 4 | 4, the third mask unsorted
  nice    d = 5: NICE 3 first | 2 | (4, NICE 3)
  elem    d = 5: (3, 2) | NormalizationLayer | (3, 4) — an element of two layers FIRST
          (have_acc false, first_in_elem and last_in_elem each true and false), a
          NormalizationLayer behind it (an element of its own), an element of two behind
          that (have_acc true)
Every three- and four-output net so runs as an s- and as a t-phase at hidden 64 and 32.

Tile settings (DF_TILES when the handle is created): 2, and 4 where the model's plan has
room for four tiles per wave (pair_tree_pin_meta.json keeps the plan's maximum from the
launch line of the generating build; d = 6 and 7 at hidden 64 stop at 2).  Per launch the
meta file also keeps the kernel and the tiles per wave it ran.  Batches, S = 128 · tiles:
1, 15, 16, 17, 31, 32, 33, S + 1 and S + 17 (there the last tile group's second tile is
wholly past the batch end).

Per model and batch: forward x / ldj, inverse x / ldj, per-sample logpdf; forward! is not
stored, its x equals forward's bit for bit (asserted here and in the test).  A launch's
per-sample bits do not depend on the tile count, so those are kept per batch: in full for
batches up to FULL_MAX and as SHA-256 of the array's bytes above.  The fp64 NLL partial sum
adds per workgroup, so it is kept per (tiles, batch).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_tail_pin as T  # noqa: E402

PARENT = "399df44"
PASSES = T.PASSES
FULL_MAX = 300
TILES = (2, 4)
_SHAPES = {
    # name: (d, elements, runs on the specialised SPLIT kernel)
    "d5": (5, [[("rnvp", [1, 2])], [("rnvp", [3, 4, 5])], [("rnvp", [4, 5])], [("rnvp", [1, 2, 3])]], True),
    "d7": (7, [[("rnvp", [1, 2, 3])], [("rnvp", [4, 5, 6, 7])]], False),
    "d8": (8, [[("rnvp", [1, 2, 3, 4])], [("rnvp", [5, 6, 7, 8])]], False),
    "d6": (6, [[("rnvp", [1, 2, 3])], [("rnvp", [4, 5, 6])], [("rnvp", [2, 4, 6])]], True),
    "d7q": (7, [[("rnvp", [1, 2, 3, 4])], [("rnvp", [4, 5, 6, 7])], [("rnvp", [7, 5, 3, 1])]], True),
    "nice": (5, [[("nice", [3, 4, 5])], [("rnvp", [1, 2])], [("rnvp", [2, 3, 4, 5]), ("nice", [5, 1, 3])]], True),
    "elem": (5, [[("rnvp", [1, 2, 3]), ("rnvp", [4, 5])], "norm", [("rnvp", [3, 5, 4]), ("rnvp", [1, 2, 4, 5])]], True),
}
# name: (d, hidden, seed, elements, specialised)
MODELS = {f"h{h}_{k}": (d, h, 400 + 10 * i + (h == 32), els, spl)
          for i, (k, (d, els, spl)) in enumerate(_SHAPES.items()) for h in (64, 32)}
NORM_BOUNDS = (np.array([-3.0, -2.5, -4.0, -3.5, -2.0], np.float32), np.array([3.5, 2.0, 3.0, 4.0, 2.5], np.float32))


def batches(tiles):
    S = T.samples_per_block(tiles)
    return (1, 15, 16, 17, 31, 32, 33, S + 1, S + 17)


def tile_settings(name, max_tiles):
    """The tiles per wave a model's launches are forced to (DF_TILES): those of TILES its plan
    has room for (max_tiles: the plan's maximum per model, as the generating build printed it).
    The chains off the specialised kernel take the setting as their kernel takes it."""
    return [t for t in TILES if t <= max_tiles[name] or not MODELS[name][4]]


def path(name):
    return os.path.join(HERE, f"pair_tree_pin_{name}.npz")


def meta():
    with open(os.path.join(HERE, "pair_tree_pin_meta.json")) as f:
        return json.load(f)


def build_model(name):
    import bench
    import densityflows_amd as dfa

    d, hidden, seed, elements, _ = MODELS[name]
    rng = np.random.default_rng(seed)
    kinds = {"rnvp": dfa.RNVPCouplingLayer, "nice": dfa.NICECouplingLayer}
    els, flat = [], []
    for e in elements:
        if e == "norm":
            els.append(dfa.NormalizationLayer(NORM_BOUNDS[0][:d], NORM_BOUNDS[1][:d], -1.0, 1.0))
            continue
        ls = [dfa.CouplingLayer(kinds[k], d, m, hidden_dim=hidden, rng=rng) for k, m in e]
        flat += ls
        els.append(ls[0] if len(ls) == 1 else dfa.FlowChain(*ls))
    bench._init_nets(dfa.FlowChain(*flat), rng)
    return dfa.FlowChain(*els)


def compile_model(name):
    """A fresh handle (the plan reads DF_TILES when it is created)."""
    hc = build_model(name).hip(device=0, n_hint=0)
    assert (hc.info.kernel == 4) == MODELS[name][4], (name, hc.info.kernel)  # 4: the specialised SPLIT kernel
    return hc


def inputs(name, B):
    """z and the inverse / logpdf input x, flat and sample-major."""
    d, _, seed, _, _ = MODELS[name]
    rng = np.random.default_rng(1000 * seed + B)
    z = rng.standard_normal((B, d)).astype(np.float32).reshape(-1)
    x = rng.standard_normal((B, d)).astype(np.float32).reshape(-1)
    return z, x


def passes(hc, name, B):
    """The pinned arrays of one model at one batch size, forward!'s x (fwdi_x) and the
    fp64 NLL partial sum (nll, one float64) beside them."""
    import torch

    dev = torch.device("cuda", 0)
    z, xin = inputs(name, B)
    tz, tx = torch.from_numpy(z).to(dev), torch.from_numpy(xin).to(dev)
    x, ldj = torch.empty_like(tz), torch.empty(B, device=dev)
    hc.run("forward", tz, None, x, ldj, B)
    zi = tz.clone()
    hc.run_inplace(zi, None, B)
    zb, ldjb, lp = torch.empty_like(tx), torch.empty(B, device=dev), torch.empty(B, device=dev)
    hc.run("backward", tx, None, zb, ldjb, B)
    hc.run_logpdf(tx, None, lp, B)
    s = torch.zeros(1, dtype=torch.float64, device=dev)
    hc.run_logpdf_sum(tx, None, s, B)
    torch.cuda.synchronize()
    got = dict(zip(PASSES, (x, ldj, zb, ldjb, lp)))
    got["fwdi_x"], got["nll"] = zi, s
    return {k: v.cpu().numpy() for k, v in got.items()}


def pinned(a, B):
    """What the pin file holds for array a of batch B: the array, or its SHA-256."""
    return a if B <= FULL_MAX else T.digest(a)


def launches(ran):
    """[kernel, tiles per wave] of every launch line, in order."""
    return [[k, int(t)] for _, _, k, t, _ in ran]


def main():
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unstated"
    assert commit.startswith(PARENT), f"the pins come from a build of {PARENT}, not {commit}"
    total, kernels, max_tiles = 0, {}, {}
    os.environ["DF_DEBUG_LAUNCH"] = "1"
    for name in MODELS:
        os.environ["DF_TILES"] = "2"
        hc = compile_model(name)
        _, ran = T.launch_lines(lambda: passes(hc, name, 17))
        max_tiles[name] = int(ran[0][4])
        out, seen = {}, set()
        for tiles in tile_settings(name, max_tiles):
            os.environ["DF_TILES"] = str(tiles)
            hc = compile_model(name)
            for B in batches(tiles):
                got, ran = T.launch_lines(lambda: passes(hc, name, B))
                assert len(ran) >= 4, (name, tiles, B, ran)
                if MODELS[name][4]:
                    assert all(k == "uniform-fast-split" and int(t) == tiles for _, _, k, t, _ in ran), (name, B, ran)
                kernels[f"{name}_t{tiles}_{B}"] = launches(ran)
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
    with open(os.path.join(HERE, "pair_tree_pin_meta.json"), "w") as f:
        json.dump({"commit": commit, "models": sorted(MODELS), "max_tiles": max_tiles, "kernels": kernels,
                   "full_max": FULL_MAX}, f, indent=1)
        f.write("\n")
    print("wrote", len(MODELS), "models,", total, "bytes, commit", commit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
