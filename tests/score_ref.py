"""fp64 analytic reference of the per-sample input gradients of logpdf.

``logpdf_grad(spec, x, θ[, tmin, tmax])`` is the oracle's ``nll_and_grad`` sweep with the
seed z̄ = -z, j̄ = 1, nothing summed over the batch and the θ rows of the conditioner-input
cotangent kept (rrule(RNVP_backward)'s ū, src/affine/RNVP.jl:137-141; NICE.jl:102-111).
It also returns, per sample, the smallest |pre-activation| over all relu / leakyrelu
Denses: the distance to the nearest kink, where an f32 evaluation may legitimately take
the other branch of σ'.
"""
import numpy as np

from oracle import flow_oracle as O

_KINKED = ("relu", "leakyrelu")


def _kink(net, cache, kink):
    for layer, (_, pre, _) in zip(net, cache):
        if layer["act"] in _KINKED:
            kink = np.minimum(kink, np.min(np.abs(pre), axis=0))
    return kink


def logpdf_grad(spec, x, theta, tmin=None, tmax=None, dtype=np.float64):
    """(lp (B,), gx (d, B), gθ (n, B), kink (B,)).  θ is used as given, or, with bounds,
    is raw: normalised first (normalize_input), and gθ is the gradient in the raw θ
    (gθ_n / (max - min), 0 where max == min)."""
    layers = O._flat_layers(spec)
    x = np.asarray(x, dtype=dtype)
    B = x.shape[1]
    th = np.asarray(theta, dtype=dtype).reshape(-1, B)
    n = th.shape[0]
    scale = None
    if tmin is not None:
        lo = np.asarray(tmin, dtype=dtype).reshape(-1, 1)
        diff = np.asarray(tmax, dtype=dtype).reshape(-1, 1) - lo
        const = diff[:, 0] == 0
        safe = np.where(diff == 0, 1.0, diff)
        th = (th - lo) / safe
        th[const, :] = 0
        scale = np.where(diff == 0, 0.0, 1.0 / safe)
    u = x
    saved = []
    ldj = np.zeros(B, dtype=dtype)
    kink = np.full(B, np.inf, dtype=dtype)
    for L in reversed(layers):  # inverse pass, last layer first (src/Chains.jl:149-165)
        if L["kind"] == "norm":
            saved.append((L, u, None))
            u, l = O.norm_backward(L, u, th, dtype)
            ldj = ldj + l
            continue
        inp = O._conditioner_input(L, u, th, dtype)
        t, tcache = O._mlp_forward_cache(L["t_net"], inp, dtype)
        kink = _kink(L["t_net"], tcache, kink)
        if L["kind"] == "rnvp":
            s, scache = O._mlp_forward_cache(L["s_net"], inp, dtype)
            kink = _kink(L["s_net"], scache, kink)
        else:
            s, scache = np.zeros_like(t), None
        af = np.asarray(L["axis_af"], dtype=np.int64) - 1
        z = u.copy()
        z[af, :] = (u[af, :] - t) * np.exp(-s)
        saved.append((L, u, (s, t, scache, tcache, af)))
        if L["kind"] == "rnvp":
            ldj = ldj - O._ldj_sum(s)
        u = z
    z = u
    lp = O.mvnormal_logpdf(z, dtype) + ldj
    zbar = -z          # ∂ logpdf(MvNormal(0, I), z) / ∂z
    jbar = 1.0         # ∂ lp / ∂ ldj
    thbar = np.zeros((n, B), dtype=dtype)
    for L, u_in, extra in reversed(saved):  # chain order
        if L["kind"] == "norm":
            xmin = np.asarray(L["x_min"], dtype=dtype)[:, None]
            xmax = np.asarray(L["x_max"], dtype=dtype)[:, None]
            zbar = zbar * (dtype(L["beta"]) - dtype(L["alpha"])) / (xmax - xmin)
            continue
        s, t, scache, tcache, af = extra
        e = np.exp(-s)
        zbar_af = zbar[af, :]
        sbar = -zbar_af * (u_in[af, :] - t) * e - jbar   # = -z̄_af·z_af - j̄
        tbar = -zbar_af * e
        ubar = zbar.copy()
        ubar[af, :] = zbar_af * e
        g_in, _ = O._mlp_backward(L["t_net"], tcache, tbar, dtype)
        if L["kind"] == "rnvp":
            g_s, _ = O._mlp_backward(L["s_net"], scache, sbar, dtype)
            g_in = g_in + g_s
        # g_in is the cotangent of vcat(θ, u)[axis_nn]
        for kk, slot in enumerate(np.asarray(L["axis_nn"], dtype=np.int64) - 1):
            if slot >= L["n"]:
                ubar[slot - L["n"], :] += g_in[kk, :]
            else:
                thbar[slot, :] += g_in[kk, :]
        zbar = ubar
    if scale is not None:
        thbar = thbar * scale
        thbar[scale[:, 0] == 0, :] = 0.0
    return lp, zbar, thbar, kink


def pre_spec(rng, act, n=2):
    """The construction of tests/test_score_ref.py: d = 5, RNVP masks [4,2,5] and [1,3], a
    block on [2,5,1,3], a NICE layer on [1,3] and NormalizationLayer(x, -1, 1); hidden 16,
    bias_scale 0.1, out_scale 0.5.  ``act``: one activation, or one per coupling layer."""
    acts = [act] * 5 if isinstance(act, str) else list(act)
    kw = dict(hidden=16, bias_scale=0.1, out_scale=0.5)
    ax = lambda m: O.coupling_axes(5, m, n=n)
    b1 = ax([2, 5, 1, 3])
    nice = O.rnvp_layer(rng, ax([1, 3]), act=acts[4], **kw)
    nice["kind"] = "nice"
    del nice["s_net"]
    return {"kind": "chain", "layers": [
        O.rnvp_layer(rng, ax([4, 2, 5]), act=acts[0], **kw),
        O.rnvp_layer(rng, ax([1, 3]), act=acts[1], **kw),
        {"kind": "block", "layer_1": O.rnvp_layer(rng, b1, act=acts[2], **kw),
         "layer_2": O.rnvp_layer(rng, O.reverse_axes(b1), act=acts[3], **kw)},
        nice,
        {"kind": "norm", "x_min": np.full(5, -3.0, np.float32), "x_max": np.full(5, 2.5, np.float32),
         "alpha": -1.0, "beta": 1.0},
    ]}
