"""Chains, inputs and cases of the training edge matrix ("training edge matrix").

numpy and the oracle only: tests/test_train_edges_host.py imports this module without the
library.  The spec builders are the ones tests/test_gpu_train.py and tests/test_gpu_score.py
have always used (they import them back from here); CASES names one case per training
kernel instance that has a batch loop of its own, with the reverse-sweep form it must run.

The persistent training kernels size their grid from the CU count and walk the batch in a
loop, so on a whole chip a wave makes a second trip only past 32 768 samples.
`DF_GRID_CUS` (read at df_chain_create) sizes those grids from a CU count of the test's
choice; batches() lists the batches around the samples P that one trip of a kernel covers.
"""
import numpy as np

from oracle import flow_oracle as O
import score_ref as R

G_RTOL = 1e-4
G_ATOL = 2e-5


def _flat_oracle_grads(spec, grads):
    parts = []
    for L, g in zip(O._flat_layers(spec), grads):
        if L["kind"] == "norm":
            continue
        for net in ("s_net", "t_net"):
            if net not in L:
                continue
            for (dW, db), D in zip(g[net], L[net]):
                parts.append(np.asarray(dW).ravel(order="F"))
                if D.get("b") is not None:
                    parts.append(np.asarray(db))
    return np.concatenate(parts)


def _tensor_slices(spec):
    out, o = [], 0
    for L in O._flat_layers(spec):
        if L["kind"] == "norm":
            continue
        for net in ("s_net", "t_net"):
            for D in L.get(net, []):
                out.append(slice(o, o + D["W"].size))
                o += D["W"].size
                if D.get("b") is not None:
                    out.append(slice(o, o + D["b"].size))
                    o += D["b"].size
    return out


def _readme_spec(rng, hidden=16):
    """test/runtests.jl:103-109: three RNVP layers + NormalizationLayer(x, -1, 1)."""
    layers = [O.rnvp_layer(rng, O.coupling_axes(5, m, n=1), hidden=hidden, bias_scale=0.1, out_scale=0.5)
              for m in ([1, 2, 3], [3, 4, 5], [5, 1, 2])]
    layers.append({"kind": "norm", "x_min": np.full(5, -3.0, np.float32), "x_max": np.full(5, 2.5, np.float32),
                   "alpha": -1.0, "beta": 1.0})
    return {"kind": "chain", "layers": layers}


def _cfg2_spec(rng):
    """BASELINE configs[1]: FlowChain(CouplingBlock, 4, 5; hidden 64), n = 0."""
    blocks = []
    for _ in range(4):
        blocks.append(O.coupling_block(rng, O.coupling_axes_cut(5, n=0), hidden=64, bias_scale=0.1,
                                       out_scale=0.1))
    return {"kind": "chain", "layers": blocks}


def _mixed_spec(rng):
    """tanh / sigmoid conditioners, n_sublayers = 1, a NICE layer, hidden 32."""
    nice = O.rnvp_layer(rng, O.coupling_axes(6, [2, 5], n=2), hidden=32, act="tanh", bias_scale=0.1)
    nice["kind"] = "nice"
    del nice["s_net"]
    return {"kind": "chain", "layers": [
        O.rnvp_layer(rng, O.coupling_axes(6, [1, 3, 6], n=2), hidden=32, act="tanh", bias_scale=0.1,
                     out_scale=0.5),
        nice,
        O.coupling_block(rng, O.coupling_axes_cut(6, 2, n=2), n_sub=1, hidden=32, act="sigmoid",
                         bias_scale=0.1, out_scale=0.5),
    ]}


def _wide_spec(rng):
    """hidden 256 (the layer-wise path): a conditioned 8-d chain with MFMA-sized
    outputs (4 transformed dims), a 3-Dense-hidden net and tanh."""
    return {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(8, 4, n=3), hidden=256, bias_scale=0.1, out_scale=0.1),
        O.rnvp_layer(rng, O.coupling_axes(8, [2, 4, 6, 8, 1], n=3), n_sub=3, hidden=128, act="tanh",
                     bias_scale=0.1, out_scale=0.2),
        {"kind": "norm", "x_min": np.full(8, -3.0, np.float32), "x_max": np.full(8, 3.5, np.float32),
         "alpha": 0.0, "beta": 1.0},
    ]}


def _cfg5_spec(rng):
    """BASELINE configs[3]/[4] model: FlowChain(CouplingBlock, 8, 32; n = 8, hidden 256)."""
    return {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(32, n=8), hidden=256, bias_scale=0.1, out_scale=0.1)
        for _ in range(8)]}


def _cfg5_in40_spec(rng):
    """config-5-sized nets whose first Dense takes 40 inputs (d = 32, n = 24): the wide
    SPLIT kernel runs the inverse pass, but the H0-free sweep's 32-float feature rows do
    not hold them."""
    return {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(32, n=24), hidden=256, bias_scale=0.1, out_scale=0.1)
        for _ in range(2)]}


def _cfg5_in52_spec(rng):
    """One config-5-sized block whose first Dense takes 52 inputs (d = 16, n = 44: 8 identity
    dims + 44 conditions, 8 transformed dims, n + d = 60 <= 64): the reverse sweep's x̄ = W0ᵀδ0
    runs apart from the W1ᵀδ1 launch.  w1t_delta_xbar (df_lsweep.hip) keeps W0ᵀ resident
    beside the 96 KiB of SPLIT W1ᵀ chunk buffers; with 49-64 inputs W0ᵀ has four 16-row tiles,
    so its split planes cost 8 · 4 · 3 KiB = 96 KiB and its f32 fragments 4 · 16 · 1 KiB =
    64 KiB: 96 + 64 KiB (+ 64 B of column table) passes the 160 KiB of LDS, the function
    returns false, and a plain δ0 launch is followed by an x̄-only product.  (40 inputs: three
    tiles, 96 + 48 KiB, resident.)"""
    return {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(16, n=44), hidden=256, bias_scale=0.1, out_scale=0.1)]}


def _cfg5x2_spec(rng):
    """Two config-5 blocks (the _cfg5_in40_spec pattern with n = 8): every net is the H0-free
    sweep's shape, at a quarter of config 5's oracle cost."""
    return {"kind": "chain", "layers": [
        O.coupling_block(rng, O.coupling_axes_cut(32, n=8), hidden=256, bias_scale=0.1, out_scale=0.1)
        for _ in range(2)]}


PRE_ACTS = ["softplus", "swish", "logcosh", "softplus", "swish"]


def _pre_spec(rng):
    """tests/score_ref.py's construction with activations whose σ' needs the pre-activation
    (the fused kernels' AM_PRE instances)."""
    return R.pre_spec(rng, PRE_ACTS, n=2)


SPECS = {"readme": (_readme_spec, 5, 1), "cfg2": (_cfg2_spec, 5, 0), "mixed": (_mixed_spec, 6, 2),
         "wide": (_wide_spec, 8, 3), "cfg5": (_cfg5_spec, 32, 8), "cfg5_in40": (_cfg5_in40_spec, 32, 24),
         "cfg5_in52": (_cfg5_in52_spec, 16, 44)}

# the edge matrix's own chains (kept out of SPECS, which tests/test_gpu_train.py extends)
EDGE_SPECS = dict(SPECS, cfg5x2=(_cfg5x2_spec, 32, 8), pre=(_pre_spec, 5, 2))


def _inputs(d, n, B, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((d, B)).astype(np.float32)
    th = rng.random((n, B)).astype(np.float32) if n > 0 else np.zeros((0, B), np.float32)
    return x, th


# ---------------------------------------------------------------------------
# the training edge matrix
# ---------------------------------------------------------------------------

# case → (chain, requested sweep form, the form it must run, environment at df_chain_create).
# One per kernel instance with a loop body of its own:
#   readme        train_net_kernel, relu (AM_RELU), exact f32
#   readme_lw     the layer-wise kernels on small nets, activations recomputed
#   cfg2          train_net_kernel's SPLIT instance (hidden 64)
#   cfg2_exact    ... and its exact-f32 one
#   mixed         tanh / sigmoid (AM_Y), a NICE layer, n_sublayers = 1
#   pre           softplus / swish / logcosh (AM_PRE): σ' held in registers across the tile
#   wide_*        hidden 256 and a 3-hidden-Dense tanh net: kept H and recomputed H
#   cfg5x2_*      config-5 nets: H0-free (ldw_split<H0R>, LEPI_DACT_XBAR_MASK), kept,
#                 recomputed, and exact f32 (no SPLIT planes anywhere)
#   cfg5_in52     x̄ = W0ᵀδ0 apart from the W1ᵀδ1 launch
CASES = {
    "readme": ("readme", "AUTO", "FUSED", {}),
    "readme_lw": ("readme", "LAYERWISE", "RECOMPUTE", {}),
    "cfg2": ("cfg2", "AUTO", "FUSED", {}),
    "cfg2_exact": ("cfg2", "AUTO", "FUSED", {"DF_F32_EXACT": "1"}),
    "mixed": ("mixed", "AUTO", "FUSED", {}),
    "pre": ("pre", "AUTO", "FUSED", {}),
    "wide_kept": ("wide", "AUTO", "KEPT", {}),
    "wide_recompute": ("wide", "RECOMPUTE", "RECOMPUTE", {}),
    "cfg5x2_h0free": ("cfg5x2", "AUTO", "H0FREE", {}),
    "cfg5x2_kept": ("cfg5x2", "KEPT", "KEPT", {}),
    "cfg5x2_recompute": ("cfg5x2", "RECOMPUTE", "RECOMPUTE", {}),
    "cfg5x2_exact": ("cfg5x2", "AUTO", "KEPT", {"DF_F32_EXACT": "1"}),
    "cfg5_in52": ("cfg5_in52", "AUTO", "KEPT", {}),
}

# chains of the score (df_train_logpdf_grad) matrix with the relu-kink caps
# tests/test_gpu_score.py uses for each
SCORE_CASES = {"readme": 0.02, "cfg2": 0.10, "mixed": 0.0, "pre": 0.0}

B_LIMIT = 2000          # every batch of the matrix stays below it (a few seconds per case)
GRID_CUS = 2            # two workgroups: reduce_grads and r · gridDim.x + blockIdx.x stay non-trivial
GRID_CUS_ODD = 3        # one more run at the largest batch: ranges off the tile / 32-sample grid
# 3 · 512 + 17: in ldense's fourth round only some waves of one workgroup have a valid
# tile, every other wave runs the all-padding path
LAYERWISE_EXTRA = (1553,)


def batches(trips, extra=()):
    """The batches around every trip size P (samples one pass of a kernel's batch loop
    covers): P − 1, P, P + 1, 2P + 17 and 3P + 53, deduplicated, below B_LIMIT."""
    out = set(extra)
    for P in trips:
        out.update((P - 1, P, P + 1, 2 * P + 17, 3 * P + 53))
    return sorted(b for b in out if 0 < b < B_LIMIT)


def fused_trips(grid):
    """train_net_kernel: gridDim.x workgroups of 8 waves, a 16-sample tile per wave and trip."""
    return (grid * 8 * 16,)


def layerwise_trips(lgrid):
    """couple_body (the front): nb · 8 tiles per trip; ldense_kernel: 8 waves · kLTiles = 2
    tiles per workgroup and round.  (The ldw loops step 32 or 64 samples through a range of
    ceil(B / lgrid) samples: any batch here gives them several steps.)"""
    return (lgrid * 8 * 16, lgrid * 8 * 2 * 16)


def score_trips(grid):
    """score_net_kernel: gridDim.x workgroups of 4 waves, a 16-sample tile per wave and trip."""
    return (grid * 4 * 16,)


def largest_batches(form):
    """The largest batch a case of this form can run at GRID_CUS CUs: the fused kernel holds
    1 to 4 workgroups of 8 waves per CU, the layer-wise grids are one workgroup per CU.
    tests/test_train_edges_host.py shows at each that a lost tile fails the value check."""
    if form == "FUSED":
        return sorted({batches(fused_trips(GRID_CUS * occ))[-1] for occ in (1, 2, 3, 4)})
    return [batches(layerwise_trips(GRID_CUS), LAYERWISE_EXTRA)[-1]]


_DATA = {}


def case_data(chain):
    """(spec, d, n, x, θ) of a chain: weights from default_rng(0), B_LIMIT samples; every
    batch of the matrix is a prefix.  Built once and shared, never modified."""
    if chain not in _DATA:
        make, d, n = EDGE_SPECS[chain]
        spec = make(np.random.default_rng(0))
        x, th = _inputs(d, n, B_LIMIT)
        _DATA[chain] = (spec, d, n, x, th)
    return _DATA[chain]


_REF = {}


def oracle_grad(chain, B, drop_last_tile=False):
    """(loss, flat fp64 gradient) of the first B samples — with drop_last_tile, of all but
    the last 16 of them under the full batch's 1/B — computed once per (chain, B)."""
    key = (chain, B, drop_last_tile)
    if key not in _REF:
        spec, d, n, x, th = case_data(chain)
        m = B - 16 if drop_last_tile else B
        loss, g = O.nll_and_grad(spec, x[:, :m], th[:, :m], n_total=B)
        _REF[key] = (loss, _flat_oracle_grads(spec, g))
    return _REF[key]



# Inputs of the score matrix: default_rng(5).  The caps of SCORE_CASES bound the share of
# samples the fp64 reference itself puts within 1e-5 of a relu kink; with this seed the
# reference keeps them at every batch the matrix can run (one to eight score workgroups per
# CU: at most 1.6 % for readme, 7.1 % for cfg2; seed 1 gives cfg2 13 % at B = 128).
SCORE_SEED = 5
_SCORE = {}


def score_data(chain):
    """(spec, x, θ, reference (lp, gx, gθ, kink)) over B_LIMIT samples.  Per-sample
    quantities: the reference of a batch B is its first B columns."""
    if chain not in _SCORE:
        spec, d, n, _, _ = case_data(chain)
        x, th = _inputs(d, n, B_LIMIT, seed=SCORE_SEED)
        _SCORE[chain] = (spec, x, th, R.logpdf_grad(spec, x, th))
    return _SCORE[chain]
