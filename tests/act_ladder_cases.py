"""Chains, inputs and cases of the activation ladder ("activation ladder and
isolation matrix").  numpy and the oracle only: tests/test_act_ladder_host.py imports this
module without the library, tests/test_gpu_act_ladder.py runs the same cases on the device.

Glorot weights, `bias_scale=0.1` and N(0, 1) inputs keep every pre-activation of the other
test chains within a few units of zero, where tanh_fast never saturates, sigmoid_fast never
clamps and the overflow-safe forms of softplus / logcosh are not needed.  A *ladder net*
puts the branch points into the biases instead, so that they are met whatever the data:

  Dense(in, h, σ)      W = 0.25 · glorot, b = a seeded permutation of LADDER tiled to h
  Dense(h, h, σ) ...   W = glorot / (1 + max|h_prev|), b = another permutation
  Dense(h, out, σ_out) W = glorot / max(1, max|W·h|), b = U(±0.1)

(both maxima over the case's own inputs, in fp64).  The input-driven part of a
pre-activation is then a jitter of order 0.1 … 1 around each ladder point, and |s| ≲ 1.1.
Where σ_out is not the identity, the last Dense's biases are ladder points c with
|σ_out(c)| ≤ 3 (so exp(s) stays finite): the points the branch regions of
tests/test_act_ladder_host.py are anchored at first, then the others in a seeded order, dealt
out over the nets of the chain; and the rows of that W are made orthogonal to the mean hidden
vector, because W·h of hidden units parked at ladder points is mostly a constant, which
would move every output pre-activation off its point by up to 1.

A chain is built layer by layer: each layer's rescale sees the fp64 output of the layers
before it on the case's inputs z; x_in, the input of the inverse, logpdf, training and
score passes, is the rounded fp64 forward of z, so those passes meet the same
pre-activations.
"""
import math

import numpy as np

from oracle import flow_oracle as O
import score_ref as R
from train_edge_cases import G_ATOL, G_RTOL, _flat_oracle_grads, _tensor_slices  # noqa: F401  (re-exported)

LADDER = np.array([-100, -88, -80, -60, -40, -20, -10, -8.124, -5, -2, -1, -0.5, -0.25, -0.1, -1e-3, 1e-3,
                   0.1, 0.25, 0.5, 1, 2, 3, 5, 8.124, 10, 17, 20, 40, 60, 80, 88, 100], np.float32)
assert LADDER.size == 32 and abs(math.sqrt(66.0) - 8.12404) < 1e-5

# the ladder points the branch regions are anchored at (REGIONS below), in dealing order
_KEY = (8.124, -8.124, 40, -80, 100, -100, 1e-3, -1e-3, 1, -1, 88, -88, 2, -2)

# Branch regions of the non-relu activation code: (name, predicate on the fp64
# pre-activations, ladder points a visit can come from).  A region is required of an
# activation wherever one of its anchors may be a bias of a Dense with that activation.
REGIONS = (
    ("x2<66, x>8", lambda p: (p * p < 66) & (p > 8), (8.124,)),
    ("x2<66, x<-8", lambda p: (p * p < 66) & (p < -8), (-8.124,)),
    ("x2>=66, x<8.3", lambda p: (p * p >= 66) & (p > 0) & (p < 8.3), (8.124,)),
    ("x2>=66, x>-8.3", lambda p: (p * p >= 66) & (p < 0) & (p > -8.3), (-8.124,)),
    ("40<x<40.5", lambda p: (p > 40) & (p < 40.5), (40,)),
    ("39.5<x<=40", lambda p: (p > 39.5) & (p <= 40), (40,)),
    ("-80.5<x<-80", lambda p: (p > -80.5) & (p < -80), (-80,)),
    ("-80<=x<-79.5", lambda p: (p >= -80) & (p < -79.5), (-80,)),
    ("|x|>88", lambda p: np.abs(p) > 88, (100, -100, 88, -88)),
    ("|x|<2e-3", lambda p: np.abs(p) < 2e-3, (1e-3, -1e-3)),
    ("1<=|x|<=5", lambda p: (np.abs(p) >= 1) & (np.abs(p) <= 5), (1, -1, 2, -2, 3, 5, -5)),
)

ALL_ACTS = ("tanh", "sigmoid", "softplus", "logcosh", "leakyrelu", "elu", "swish", "relu")
OUT_ACTS = ("tanh", "sigmoid", "softplus", "elu")
SMOOTH = ("tanh", "sigmoid", "softplus", "logcosh", "elu", "swish")
LW_ACTS = ("tanh", "softplus", "elu")
FIRST_SCALE = 0.25

README_MASKS = ([1, 2, 3], [3, 4, 5], [5, 1, 2])


def out_pool(act):
    """The ladder points a last Dense with activation ``act`` may have as a bias."""
    v = O.activation(act, LADDER.astype(np.float64))
    return LADDER[np.abs(v) <= 3.0]


def _perm_bias(rng, h):
    reps = -(-h // LADDER.size)
    return np.concatenate([LADDER[rng.permutation(LADDER.size)] for _ in range(reps)])[:h].astype(np.float32)


class _OutDeal:
    """Deals the pool of an output activation over the nets of one chain: the anchors of
    the branch regions first, then the other points in a seeded order, then again."""

    def __init__(self, rng, act):
        pool = out_pool(act)
        key = [np.float32(k) for k in _KEY if np.any(pool == np.float32(k))]
        rest = [c for c in pool[rng.permutation(pool.size)] if not any(c == k for k in key)]
        self.order, self.at = np.array(key + rest, np.float32), 0

    def take(self, count):
        idx = (self.at + np.arange(count)) % self.order.size
        self.at += count
        return self.order[idx].copy()


def ladder_net(rng, inp, dims, acts, deal=None):
    """A ladder net of Dense(dims[i], dims[i+1], acts[i]) scaled for the fp64 inputs ``inp``
    (dims[0], B).  ``deal``: the _OutDeal of a chain whose output activation is acts[-1]."""
    net, h = [], np.asarray(inp, np.float64)
    last = len(dims) - 2
    for i in range(len(dims) - 1):
        W = O.glorot_uniform(rng, dims[i + 1], dims[i]).astype(np.float64)
        if i == 0 and i != last:
            W = W * FIRST_SCALE
            b = _perm_bias(rng, dims[1])
        elif i != last:
            W = W / (1.0 + float(np.max(np.abs(h))))
            b = _perm_bias(rng, dims[i + 1])
        else:
            if acts[i] != "identity":
                # the hidden units sit at their ladder points, so W·h is a constant of order
                # 1 plus a small jitter: take the constant out (rows orthogonal to the mean
                # h), or no output pre-activation would stay near its own ladder point
                hm = np.mean(h, axis=1)
                W = W - np.outer(W @ hm, hm) / float(hm @ hm)
            W = W / max(1.0, float(np.max(np.abs(W @ h))))
            u = ((rng.random(dims[i + 1]) * 2 - 1) * 0.1).astype(np.float32)
            b = u if acts[i] == "identity" else deal.take(dims[i + 1])
        D = {"W": W.astype(np.float32), "b": b.astype(np.float32), "act": acts[i]}
        net.append(D)
        h = O.dense(D, h, np.float64)
    return net


def _norm(rng, d):
    lo = (-3.0 + rng.random(d)).astype(np.float32)
    hi = (2.0 + 1.5 * rng.random(d)).astype(np.float32)
    return {"kind": "norm", "x_min": lo, "x_max": hi, "alpha": -1.0, "beta": 1.0}


def ladder_chain(rng, z, th, d, n, layers, norm):
    """layers: (kind, mask, s (dims-after-input, acts), t (dims-after-input, acts)); the nets
    of each layer are scaled on the fp64 forward of z through the layers before it."""
    out_act = layers[0][3][1][-1]
    deal = _OutDeal(rng, out_act) if out_act != "identity" else None
    u, out = np.asarray(z, np.float64), []
    for kind, mask, s_shape, t_shape in layers:
        ax = O.coupling_axes(d, mask, n=n)
        inp = O._conditioner_input(ax, u, th, np.float64)
        n_in = len(ax["axis_nn"])
        L = dict(ax, kind=kind)
        # (t-net first: O.rnvp_layer's order)
        L["t_net"] = ladder_net(rng, inp, [n_in] + list(t_shape[0]), t_shape[1], deal)
        if kind == "rnvp":
            L["s_net"] = ladder_net(rng, inp, [n_in] + list(s_shape[0]), s_shape[1], deal)
        out.append(L)
        u, _ = O.forward(L, u, th, np.float64)
    if norm:
        out.append(_norm(rng, d))
    return {"kind": "chain", "layers": out}


def _default_layers(masks, hidden, act, out_act="identity", n_hidden=2):
    shape = lambda m: ([hidden] * n_hidden + [len(m)], [act] * n_hidden + [out_act])
    kinds = ["rnvp", "nice", "rnvp"]
    return [(k, m, shape(m), shape(m)) for k, m in zip(kinds, masks)]


def _mixed_layers():
    """Hand-built nets of widths 12-32 and depths 3-4 (as edge_cases._generic_custom), no two
    Denses of a net with the same σ; every activation is the first Dense (width 32: the
    whole ladder) of one net."""
    I = "identity"
    return [
        ("rnvp", [6, 2, 4], ([32, 16, 3], ["sigmoid", "relu", I]), ([32, 12, 24, 3], ["logcosh", "swish", "relu", I])),
        ("nice", [1, 5, 3], None, ([32, 20, 3], ["tanh", "elu", I])),
        ("rnvp", [7, 3], ([32, 16, 2], ["elu", "tanh", I]), ([32, 12, 2], ["swish", "softplus", I])),
        ("rnvp", [2, 5, 6], ([32, 24, 3], ["softplus", "leakyrelu", I]), ([32, 16, 3], ["leakyrelu", "sigmoid", I])),
        ("nice", [4, 1], None, ([32, 16, 2], ["relu", "logcosh", I])),
    ]


MFMA_MASKS = ([11, 3, 7, 1, 9, 5], [2, 4, 6, 8, 10, 12], [12, 1, 6, 3, 8, 10])

# ---------------------------------------------------------------------------
# chain-pass cases: name → (d, n, B, layers, environment at df_chain_create, accepted
# df_chain_info.kernel ids, the call site the case is there for)
# ---------------------------------------------------------------------------
UNIFORM_IDS, GENERIC_IDS = (1, 2), (0,)
CHAIN_CASES = {}
for _a in ALL_ACTS:
    # relu hidden nets of the README shape are FAST chains: DF_NO_FAST keeps them on the
    # uniform kernel this case is about
    _env = {"DF_NO_FAST": "1"} if _a == "relu" else {}
    CHAIN_CASES["uni_" + _a] = (5, 1, 257, _default_layers(README_MASKS, 32, _a), _env, UNIFORM_IDS,
                                "df_uniform_impl.h hidden act_fn")
    CHAIN_CASES["gen_" + _a] = (5, 1, 257, _default_layers(README_MASKS, 32, _a), {"DF_FORCE_GENERIC": "1"},
                                GENERIC_IDS, "df_chain_impl.h hidden act_fn")
for _a in OUT_ACTS:
    CHAIN_CASES["uni_out_" + _a] = (5, 1, 257, _default_layers(README_MASKS, 32, "relu", _a), {}, UNIFORM_IDS,
                                    "df_uniform_impl.h VALU output act_fn")
    CHAIN_CASES["gen_out_" + _a] = (5, 1, 257, _default_layers(README_MASKS, 32, "relu", _a),
                                    {"DF_FORCE_GENERIC": "1"}, GENERIC_IDS, "df_chain_impl.h output act_fn")
CHAIN_CASES["mfma_out_tanh"] = (12, 2, 145, _default_layers(MFMA_MASKS, 64, "tanh", "tanh"), {}, UNIFORM_IDS,
                                "df_uniform_impl.h MFMA output act_fn")
CHAIN_CASES["gen_mixed"] = (7, 1, 257, _mixed_layers(), {}, GENERIC_IDS, "generic, per-Dense D.act dispatch")

# gradient cases: name → (layers, requested sweep, the form it must run, σ' form, environment)
TRAIN_B = 300
TRAIN_GRID_CUS = 2
GRAD_CASES = {}
for _a in SMOOTH:
    GRAD_CASES["grad_" + _a] = (_default_layers(README_MASKS, 32, _a), "AUTO", "FUSED",
                                "AM_Y" if _a in ("tanh", "sigmoid", "elu") else "AM_PRE")
GRAD_CASES["grad_out_tanh"] = (_default_layers(README_MASKS, 32, "relu", "tanh"), "AUTO", "FUSED", "AM_RELU")
LW_CHAINS = {"lw_" + _a: _default_layers(README_MASKS, 128, _a, n_hidden=3) for _a in LW_ACTS}
for _a in LW_ACTS:
    for _f in ("KEPT", "RECOMPUTE"):
        GRAD_CASES[f"lw_{_a}_{_f.lower()}"] = (LW_CHAINS["lw_" + _a], _f, _f, None)
SCORE_CASES = tuple("grad_" + a for a in SMOOTH)

# seeds: one per chain ("same chain" cases share theirs).  A case whose float32 oracle
# missed the bounds of tests/test_act_ladder_host.py would get another seed here; the
# tolerance is not what moves.
_SEED = {}
for _i, _a in enumerate(ALL_ACTS):
    _SEED["uni_" + _a] = _SEED["gen_" + _a] = _SEED["grad_" + _a] = 300 + _i
for _i, _a in enumerate(OUT_ACTS):
    _SEED["uni_out_" + _a] = _SEED["gen_out_" + _a] = 320 + _i
_SEED["grad_out_tanh"] = _SEED["uni_out_tanh"]
_SEED["mfma_out_tanh"] = 330
_SEED["gen_mixed"] = 331
for _i, _a in enumerate(LW_ACTS):
    _SEED[f"lw_{_a}_kept"] = _SEED[f"lw_{_a}_recompute"] = 340 + _i


def _inputs(seed, d, n, B):
    rng = np.random.default_rng(seed + 1000)
    z = rng.standard_normal((d, B)).astype(np.float32)
    tmin = (-1.0 - 0.5 * np.arange(n)).astype(np.float32)
    tmax = (2.0 + 1.0 * np.arange(n)).astype(np.float32)
    th_raw = (tmin[:, None] + rng.random((n, B)) * (tmax - tmin)[:, None]).astype(np.float32)
    th = O.normalize_input(th_raw, tmin, tmax)
    return z, th, th_raw, tmin, tmax


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


_CACHE = {}


def case_data(name):
    """Spec, inputs and the fp64 oracle of a chain-pass case, with the keys of
    edge_cases.case_data.  Computed once; read-only."""
    if name in _CACHE:
        return _CACHE[name]
    d, n, B, layers = CHAIN_CASES[name][:4]
    z, th, th_raw, tmin, tmax = _inputs(_SEED[name], d, n, B)
    spec = ladder_chain(np.random.default_rng(_SEED[name]), z, th, d, n, layers, norm=True)
    x, ldj = O.forward(spec, z, th, np.float64)
    x_in = x.astype(np.float32)
    zb, ldj_b = O.backward(spec, x_in, th, np.float64)
    lp = O.flow_logpdf(spec, x_in, th, np.float64)
    _CACHE[name] = _freeze(dict(spec=spec, d=d, n=n, B=B, z=z, x_in=x_in, th=th, th_raw=th_raw, tmin=tmin,
                                tmax=tmax, x=x, ldj=ldj, zb=zb, ldj_b=ldj_b, lp=lp))
    return _CACHE[name]


def grad_data(name):
    """Spec and inputs of a gradient case (no NormalizationLayer; θ as the chain takes it)
    with the fp64 loss and flat gradient, and for the score cases the fp64 (lp, gx, gθ)."""
    key = ("grad", _SEED[name], name in SCORE_CASES)
    if key in _CACHE:
        return _CACHE[key]
    d, n, B = 5, 1, TRAIN_B
    z, th, _, _, _ = _inputs(_SEED[name], d, n, B)
    spec = ladder_chain(np.random.default_rng(_SEED[name]), z, th, d, n, GRAD_CASES[name][0], norm=False)
    x = O.forward(spec, z, th, np.float64)[0].astype(np.float32)
    loss, g = O.nll_and_grad(spec, x, th)
    out = dict(spec=spec, d=d, n=n, B=B, x=x, th=th, loss=float(loss), grad=_flat_oracle_grads(spec, g))
    if name in SCORE_CASES:
        lp, gx, gth, _ = R.logpdf_grad(spec, x, th)
        out.update(lp=lp, gx=gx, gth=gth)
    _CACHE[key] = _freeze(out)
    return _CACHE[key]


def pre_activations(spec, u_in, th, dtype=np.float64):
    """{σ: every pre-activation of the Denses with that σ} over the inverse pass of x = u_in."""
    acc = {}
    u = np.asarray(u_in, dtype)
    for L in reversed(O._flat_layers(spec)):
        if L["kind"] != "norm":
            inp = O._conditioner_input(L, u, th, dtype)
            for net in ("s_net", "t_net"):
                if net in L:
                    _, cache = O._mlp_forward_cache(L[net], inp, dtype)
                    for D, (_, pre, _) in zip(L[net], cache):
                        acc.setdefault(D["act"], []).append(pre.ravel())
        u, _ = O.backward(L, u, th, dtype)
    return {a: np.concatenate(v) for a, v in acc.items()}


def bias_points(spec):
    """{σ: the set of biases of the Denses with that σ}: which regions a σ can be asked for."""
    acc = {}
    for L in O._flat_layers(spec):
        for net in ("s_net", "t_net"):
            for D in (L.get(net) or []) if L["kind"] != "norm" else []:
                acc.setdefault(D["act"], set()).update(float(np.float32(b)) for b in D["b"])
    return acc
