"""Float32 restatement, operation for operation, of the optimiser rules the device runs
(include/densityflows_hip.h, df_opt_kind) and of a chain of them, plus a float64 per-tensor
norm.  Optimisers.jl is not available to pin parity against, so the arithmetic written in
the header is the contract and this file restates it in numpy:

    dx = g;  for every rule in order: dx = rule(x, dx)  (x: the parameters before the step);
    x = x - dx

Every array is float32 and every scalar is converted to float32 first, so each numpy
operation rounds once, as the kernels' do (they are built without contraction).
"""
import numpy as np

from densityflows_amd.train import Adam, ClipGrad, ClipNorm, Descent, OptimiserChain, WeightDecay

F = np.float32


def rules_of(opt):
    return list(opt.rules) if isinstance(opt, OptimiserChain) else [opt]


def new_state(n, opt):
    """Optimisers.setup: m = v = 0 and βᵗ = β of the chain's Adam (None without one)."""
    bt = None
    for r in rules_of(opt):
        if isinstance(r, Adam):
            bt = (F(r.beta[0]), F(r.beta[1]))
    return [np.zeros(n, F), np.zeros(n, F), bt]


def norms64(v, offsets):
    """sqrt(Σ v²) per tensor [offsets[k], offsets[k+1]) in float64."""
    v = np.asarray(v, np.float64)
    return np.array([np.sqrt(np.sum(v[a:b] ** 2)) for a, b in zip(offsets[:-1], offsets[1:])], np.float64)


def clip_grad(dx, delta):
    d = F(delta)
    return np.where(dx > d, d, np.where(dx < -d, -d, dx)).astype(F)


def clip_norm(dx, omega, offsets, norms=None):
    """Per tensor: nrm > ω → dx·(ω / nrm), else dx as it is.  ``norms``: the Float32 norms to
    use (the device's own, so that only the rule is compared); default: the float64 norm
    rounded to Float32."""
    w = F(omega)
    nr = np.asarray(norms, F) if norms is not None else norms64(dx, offsets).astype(F)
    out = dx.copy()
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        if nr[k] > w:
            out[a:b] = dx[a:b] * (w / nr[k])
    return out


def weight_decay(dx, x, lam):
    return dx + F(lam) * x


def descent(dx, eta):
    return F(eta) * dx


def adam(dx, state, eta, beta, eps):
    """oracle.flow_oracle.adam_update's arithmetic on the incoming dx; m, v updated in place."""
    eta, beta, eps = F(eta), (F(beta[0]), F(beta[1])), F(eps)
    m, v, bt = state
    m[:] = beta[0] * m + (1 - beta[0]) * dx
    v[:] = beta[1] * v + (1 - beta[1]) * (dx * dx)
    return m / (1 - bt[0]) / (np.sqrt(v / (1 - bt[1])) + eps) * eta


def chain_update(x, g, opt, state, offsets, norms=None):
    """One step of the chain on flat float32 vectors: returns (x_new, dx); ``state`` (new_state)
    is updated in place, βᵗ advanced after the step.  ``norms``: see clip_norm."""
    x = np.asarray(x, F)
    dx = np.asarray(g, F).copy()
    adam_rule = None
    for r in rules_of(opt):
        if isinstance(r, ClipGrad):
            dx = clip_grad(dx, r.delta)
        elif isinstance(r, ClipNorm):
            dx = clip_norm(dx, r.omega, offsets, norms)
        elif isinstance(r, WeightDecay):
            dx = weight_decay(dx, x, r.lam)
        elif isinstance(r, Descent):
            dx = descent(dx, r.eta)
        elif isinstance(r, Adam):
            dx = adam(dx, state, r.eta, r.beta, r.epsilon)
            adam_rule = r
        else:
            raise TypeError(r)
        assert dx.dtype == F
    if adam_rule is not None:
        bt = state[2]
        state[2] = (bt[0] * F(adam_rule.beta[0]), bt[1] * F(adam_rule.beta[1]))
    return x - dx, dx


def pre_clip_dx(x, g, opt):
    """dx as it reaches the chain's ClipNorm (the rules before it applied), or None."""
    x = np.asarray(x, F)
    dx = np.asarray(g, F).copy()
    if not any(isinstance(r, ClipNorm) for r in rules_of(opt)):
        return None
    for r in rules_of(opt):
        if isinstance(r, ClipNorm):
            return dx
        if isinstance(r, ClipGrad):
            dx = clip_grad(dx, r.delta)
        elif isinstance(r, WeightDecay):
            dx = weight_decay(dx, x, r.lam)
        elif isinstance(r, Descent):
            dx = descent(dx, r.eta)
        else:
            raise TypeError(r)
    return None
