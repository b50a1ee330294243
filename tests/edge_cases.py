"""Chains and inputs of the batch-edge matrix (tests/test_gpu_batch_edges.py), one
small conditioned chain per chain-pass kernel family.  Plain numpy: the CPU pin in
tests/test_oracle.py and the GPU file import the same specs and the same inputs.

Every chain has non-zero biases, unsorted masks, a NICE layer where its family takes
one, and a NormalizationLayer last (the inverse pass starts with it)."""
import numpy as np

from helpers import random_net as _net
from oracle import flow_oracle as O

# debug name (DF_DEBUG_LAUNCH=1) of each df_chain_info.kernel id
KERNEL_NAME = {0: "generic", 1: "uniform", 2: "uniform", 3: "uniform-fast", 4: "uniform-fast-split",
               5: "wide", 6: "wide-split"}

# samples the inputs are drawn for: 2·S + 33 at the largest workgroup of the non-wide
# kernels (S = 128 · 8 tiles per wave) and of the wide kernels (S = 128)
BMAX_CHAIN = 2 * 128 * 8 + 33
BMAX_WIDE = 2 * 128 + 33


def _norm(rng, d):
    lo = (-3.0 + rng.random(d)).astype(np.float32)
    hi = (2.0 + 1.5 * rng.random(d)).astype(np.float32)
    return {"kind": "norm", "x_min": lo, "x_max": hi, "alpha": -1.0, "beta": 1.0}


def _default_chain(rng, d, n, layers, norm=True, **kw):
    """layers: ("rnvp" | "nice", mask) with default nets (O.rnvp_layer keywords in kw)."""
    out = []
    for kind, mask in layers:
        L = O.rnvp_layer(rng, O.coupling_axes(d, mask, n=n), bias_scale=0.1, **kw)
        if kind == "nice":
            L["kind"] = "nice"
            del L["s_net"]
        out.append(L)
    if norm:
        out.append(_norm(rng, d))
    return {"kind": "chain", "layers": out}


def _generic_custom(rng):
    """Hand-built conditioners of widths 12-32 and depths 3-4 (as test_nice_and_custom_nets)."""
    d, n = 7, 1
    ax1 = O.coupling_axes(d, [6, 2, 4], n=n)          # 5 inputs, 3 outputs
    ax2 = O.coupling_axes(d, [1, 5, 3], n=n)          # 5 inputs, 3 outputs
    ax3 = O.coupling_axes(d, [7, 3], n=n)             # 6 inputs, 2 outputs
    l1 = dict(ax1, kind="rnvp", s_net=_net(rng, [5, 32, 16, 3], ["sigmoid", "relu", "identity"]),
              t_net=_net(rng, [5, 12, 16, 32, 3], ["relu", "logcosh", "relu", "identity"]))
    l2 = dict(ax2, kind="nice", t_net=_net(rng, [5, 24, 20, 3], ["tanh", "relu", "identity"]))
    l3 = dict(ax3, kind="rnvp", s_net=_net(rng, [6, 16, 32, 2], ["elu", "tanh", "identity"]),
              t_net=_net(rng, [6, 32, 12, 2], ["relu", "swish", "identity"]))
    return {"kind": "chain", "layers": [l1, l2, l3, _norm(rng, d)]}


def _generic_h256(rng):
    return _default_chain(rng, 6, 2, [("rnvp", [5, 2, 3]), ("nice", [1, 6]), ("rnvp", [4, 1, 6, 2])],
                          hidden=256, act="tanh", out_scale=0.1)


def _uniform_tanh32(rng):
    return _default_chain(rng, 5, 2, [("rnvp", [4, 2]), ("nice", [1, 3, 5]), ("rnvp", [5, 1, 2])],
                          hidden=32, act="tanh", out_scale=0.5)


def _uniform_relu_in4(rng):
    """The in4_h64 shape: the second layer's 4 conditioner inputs leave no free k-slot
    for the folded bias, so the chain is not FAST."""
    return _default_chain(rng, 6, 0, [("rnvp", [1, 2, 3, 4]), ("rnvp", [6, 2]), ("nice", [3, 5, 1])],
                          hidden=64, out_scale=0.5)


def _slowcopy_d12(rng):
    """d, n > 8: the element-by-element copy-in; 6 transformed dims: the MFMA output path."""
    return _default_chain(rng, 12, 9, [("rnvp", [11, 3, 7, 1, 9, 5]), ("nice", [2, 4, 6, 8, 10, 12]),
                                       ("rnvp", [12, 1, 6, 3, 8, 10])], hidden=64, out_scale=0.5)


def _readme_shape(hidden):
    def make(rng):
        return _default_chain(rng, 5, 1, [("rnvp", [1, 2, 3]), ("nice", [3, 4, 5]), ("rnvp", [5, 1, 2])],
                              hidden=hidden, out_scale=0.5)
    return make


def _split32(rng):
    """hidden 32 (HT = 2) with two θ columns.  FAST needs a free k-slot in the one
    first-Dense k-step (at most 3 conditioner inputs) and at most 4 outputs: with n = 2
    that is d = 5 and 4 transformed dims per layer."""
    return _default_chain(rng, 5, 2, [("rnvp", [4, 2, 5, 1]), ("nice", [3, 1, 2, 5]), ("rnvp", [5, 3, 4, 2])],
                          hidden=32, out_scale=0.5)


def _wide(rng):
    return _default_chain(rng, 6, 2, [("rnvp", [5, 2, 3]), ("nice", [1, 6, 4]), ("rnvp", [4, 1, 6, 2])],
                          hidden=256, out_scale=0.1)


def _norm_only(d):
    def make(rng):
        return {"kind": "chain", "layers": [_norm(rng, d)]}
    return make


# name: (spec builder, d, n, environment at df_chain_create, accepted df_chain_info.kernel ids,
#        tiles per wave of one tile group, the plan's largest tiles per wave)
# The largest tile count is what the LDS plan gives (`tiles T (max M)` of the debug line)
# and is asserted: the parametrisation below (which cases run DF_TILES=4) follows from it.
CASES = {
    "generic_custom": (_generic_custom, 7, 1, {}, (0,), 1, 8),
    "generic_h256": (_generic_h256, 6, 2, {}, (0,), 1, 1),
    "uniform_tanh32": (_uniform_tanh32, 5, 2, {}, (1,), 1, 8),
    "uniform_relu_in4": (_uniform_relu_in4, 6, 0, {}, (1, 2), 1, 7),
    "slowcopy_d12": (_slowcopy_d12, 12, 9, {}, (1, 2), 1, 2),
    "fast16": (_readme_shape(16), 5, 1, {"DF_SMALL_MAX": "0"}, (3,), 2, 8),
    "fast64_exact": (_readme_shape(64), 5, 1, {"DF_F32_EXACT": "1"}, (3,), 2, 6),
    "split64": (_readme_shape(64), 5, 1, {}, (4,), 2, 2),
    "split32": (_split32, 5, 2, {}, (4,), 2, 6),
    "wide_exact": (_wide, 6, 2, {"DF_F32_EXACT": "1"}, (5,), 1, 1),
    "wide_split": (_wide, 6, 2, {}, (6,), 1, 1),
}
WIDE = ("wide_exact", "wide_split")
NORM_ONLY = {"norm_only_d5": (_norm_only(5), 5, 0), "norm_only_d12": (_norm_only(12), 12, 0)}

_SEED = {name: 100 + i for i, name in enumerate(list(CASES) + list(NORM_ONLY))}
_SEED["split64"] = _SEED["fast64_exact"]      # "same chain"
_SEED["wide_split"] = _SEED["wide_exact"]


def case_spec(name):
    make = (CASES.get(name) or NORM_ONLY[name])[0]
    return make(np.random.default_rng(_SEED[name]))


def case_bmax(name):
    return BMAX_WIDE if name in WIDE else BMAX_CHAIN


_CACHE = {}


def case_data(name):
    """Spec, inputs and the fp64 oracle of a case at its largest batch, computed once
    (samples are independent: every smaller batch is a prefix).  Read-only.

    z, x_in: float32 inputs of the forward and the inverse pass (x_in is the rounded fp64
    forward of z, so the inverse runs where the flow puts its data); th: θ as the chain
    takes it, th_raw with (tmin, tmax) the flow-level θ it is the normalize_input of."""
    if name in _CACHE:
        return _CACHE[name]
    entry = CASES.get(name) or NORM_ONLY[name]
    d, n = entry[1], entry[2]
    spec = case_spec(name)
    B = case_bmax(name)
    rng = np.random.default_rng(_SEED[name] + 1000)
    z = rng.standard_normal((d, B)).astype(np.float32)
    tmin = (-1.0 - 0.5 * np.arange(n)).astype(np.float32)
    tmax = (2.0 + 1.0 * np.arange(n)).astype(np.float32)
    th_raw = (tmin[:, None] + rng.random((n, B)) * (tmax - tmin)[:, None]).astype(np.float32)
    th = O.normalize_input(th_raw, tmin, tmax) if n else np.zeros((0, B), np.float32)
    x, ldj = O.forward(spec, z, th, np.float64)
    x_in = x.astype(np.float32)
    zb, ldj_b = O.backward(spec, x_in, th, np.float64)
    lp = O.flow_logpdf(spec, x_in, th, np.float64)
    out = dict(spec=spec, d=d, n=n, B=B, z=z, x_in=x_in, th=th, th_raw=th_raw, tmin=tmin, tmax=tmax,
               x=x, ldj=ldj, zb=zb, ldj_b=ldj_b, lp=lp)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[name] = out
    return out
