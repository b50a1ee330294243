"""CPU side of the activation ladder ("activation ladder and isolation matrix"):
the matrix of tests/act_ladder_cases.py proves itself before a device sees it.

1. Coverage.  For every case and every activation in it, the fp64 pre-activations over all
   Denses with that σ visit each branch region of the activation code
   (act_ladder_cases.REGIONS: both sides of tanh_fast's x² = 66 at both signs, both sides of
   sigmoid_fast's 40 and −80, |x| > 88 where exp(x) and cosh(x) overflow, |x| < 2e-3 and
   1 ≤ |x| ≤ 5).  A region is asked of a σ wherever one of the ladder points it is anchored
   at is a bias of a Dense with that σ: everywhere for a hidden σ; for an output σ, within
   the points with |σ(c)| ≤ 3.
2. The reference stays within the tolerance.  The oracle's own float32 evaluation of every
   case meets half the GPU tests' criteria against the fp64 oracle: `close(·, ·, 1e-5)` for
   x, ldj, inverse z, inverse ldj and logpdf; G_RTOL / G_ATOL per tensor for the NLL
   gradient and for gx and gθ.  This is a condition on the inputs: a case that missed it
   would get another seed, never another tolerance.  Measured worst ratios: 0.26 for the
   values (inverse z of the softplus-output chain), 0.18 for the hidden-128 softplus NLL
   gradient, 0.14 at hidden 32.
3. The matrix bites.  Four plausible wrong activations, put in place of O.activation for
   the float32 evaluation, fail the value criterion on the ladder chain (ratio > 1 or a
   non-finite output) and pass it on the chain of test_gpu_parity.py::test_activations,
   which is the gap this matrix closes:
     * tanh_fast without its saturation branch,
     * tanh_fast saturating at |x| ≥ 66 instead of x² ≥ 66,
     * softplus as log1p(exp(x)),
     * logcosh as log(cosh(x)).
   Not detectable at 1e-5 by construction, and asserted neither way: sigmoid_fast
   saturating at −40 instead of −80 (σ(−40) = 4e-18), elu through exp(x) − 1 (an absolute
   error of 6e-8 on a unit of a 32-wide Dense) and swish with exp cut off past 80
   (80 · e⁻⁸⁰ = 1e-33).
"""
import numpy as np
import pytest

import act_ladder_cases as A
import densityflows_amd as dfa
import score_ref as R
from densityflows_amd import hip
from helpers import close, spec_to_element
from oracle import flow_oracle as O

HALF = 0.5
PLAN_KEYS = ("DF_F32_EXACT", "DF_NO_WIDE", "DF_FORCE_GENERIC", "DF_NO_FAST", "DF_NO_FOLD", "DF_STAGE_KB")


def _grad_chains():
    """One gradient case per chain (kept / recompute share theirs)."""
    seen, out = set(), []
    for name in A.GRAD_CASES:
        if A._SEED[name] not in seen or name == "grad_out_tanh":
            out.append(name)
        seen.add(A._SEED[name])
    return out


def _check_coverage(what, spec, x_in, th):
    pre, points = A.pre_activations(spec, x_in, th), A.bias_points(spec)
    for act, p in pre.items():
        if act == "identity":
            continue
        have = {np.float32(c) for c in points[act]}
        asked = 0
        for region, inside, anchors in A.REGIONS:
            if not any(np.float32(c) in have for c in anchors):
                continue
            asked += 1
            assert np.any(inside(p)), f"{what}: no {act} pre-activation in the region {region}"
        assert asked >= 5, f"{what}: only {asked} regions can be asked of {act}"
        if not any(D["act"] == act for L in O._flat_layers(spec) if L["kind"] != "norm"
                   for net in ("s_net", "t_net") for D in (L.get(net) or [])[-1:]):
            assert asked == len(A.REGIONS), f"{what}: a hidden {act} misses a ladder point"


@pytest.mark.parametrize("name", list(A.CHAIN_CASES))
def test_chain_case_plans_its_kernel(name, monkeypatch):
    """Every chain-pass case plans, without a device, onto the kernel it is there for."""
    for k in PLAN_KEYS:
        monkeypatch.delenv(k, raising=False)
    d, n, B, _, env, ids, _ = A.CHAIN_CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    info = hip.validate(spec_to_element(A.case_data(name)["spec"]).layers)
    assert info.kernel in ids and (info.d, info.n) == (d, n), (name, info.kernel)
    if name == "mfma_out_tanh":
        assert info.hidden_tiles == 4


@pytest.mark.parametrize("name", list(A.CHAIN_CASES))
def test_chain_case_coverage_and_reference(name):
    D = A.case_data(name)
    assert D["z"].shape == (D["d"], D["B"]) and all(np.all(np.isfinite(D[k])) for k in ("x", "ldj", "zb", "lp"))
    _check_coverage(name, D["spec"], D["x_in"], D["th"])
    spec, th = D["spec"], D["th"]
    x, ldj = O.forward(spec, D["z"], th, np.float32)
    zb, ldj_b = O.backward(spec, D["x_in"], th, np.float32)
    lp = O.flow_logpdf(spec, D["x_in"], th, np.float32)
    ratios = {k: close(got, D[k])[1] for k, got in (("x", x), ("ldj", ldj), ("zb", zb), ("ldj_b", ldj_b), ("lp", lp))}
    print(f"LADDER-F32 {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= HALF, (name, ratios)


@pytest.mark.parametrize("name", _grad_chains())
def test_gradient_case_coverage_and_reference(name):
    D = A.grad_data(name)
    spec, x, th = D["spec"], D["x"], D["th"]
    assert np.isfinite(D["loss"]) and np.all(np.isfinite(D["grad"]))
    _check_coverage(name, spec, x, th)
    loss, g = O.nll_and_grad(spec, x, th, dtype=np.float32)
    g = A._flat_oracle_grads(spec, g)
    ratios = {"grad": max(close(g[sl], D["grad"][sl], A.G_RTOL, A.G_ATOL)[1] for sl in A._tensor_slices(spec)),
              "loss": abs(float(loss) - D["loss"]) / (1e-5 * max(1.0, abs(D["loss"])))}
    if name in A.SCORE_CASES:
        lp, gx, gth, kink = R.logpdf_grad(spec, x, th, dtype=np.float32)
        ratios.update(lp=close(lp, D["lp"])[1], gx=close(gx, D["gx"], A.G_RTOL, A.G_ATOL)[1],
                      gth=close(gth, D["gth"], A.G_RTOL, A.G_ATOL)[1])
        assert np.all(np.isinf(kink)), "a score case with a kinked activation"
    print(f"LADDER-F32 {name}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= HALF, (name, ratios)


# ---------------------------------------------------------------------------
# the matrix bites
# ---------------------------------------------------------------------------

def _rational(x):
    x2 = x * x
    with np.errstate(all="ignore"):
        return x2, x * (O._evalpoly(x2, O._TANH_FAST_N) / O._evalpoly(x2, O._TANH_FAST_D))


def _tanh_no_saturation(x):
    return _rational(x)[1].astype(x.dtype)


def _tanh_abs_66(x):
    return np.where(np.abs(x) < x.dtype.type(66), _rational(x)[1], np.sign(x)).astype(x.dtype)


def _softplus_naive(x):
    with np.errstate(all="ignore"):
        return np.log1p(np.exp(x)).astype(x.dtype)


def _logcosh_naive(x):
    with np.errstate(all="ignore"):
        return np.log(np.cosh(x)).astype(x.dtype)


MUTANTS = {"tanh_no_saturation": ("tanh", _tanh_no_saturation), "tanh_abs_66": ("tanh", _tanh_abs_66),
           "softplus_naive": ("softplus", _softplus_naive), "logcosh_naive": ("logcosh", _logcosh_naive)}


def _mutated_forward(monkeypatch, mutant, spec, z, th):
    """The float32 forward with the activation replaced (float32 only: the fp64 truth
    keeps the real one)."""
    act, wrong = MUTANTS[mutant]
    real = O.activation
    monkeypatch.setattr(O, "activation",
                        lambda name, x: wrong(x) if (name == act and x.dtype == np.float32) else real(name, x))
    try:
        with np.errstate(all="ignore"):
            return O.forward(spec, z, th, np.float32)
    finally:
        monkeypatch.setattr(O, "activation", real)


def _value_ratio(got, want):
    """The worst `close` ratio over (x, ldj); inf for a non-finite output."""
    if not all(np.all(np.isfinite(g)) for g in got):
        return float("inf")
    return max(close(g, w)[1] for g, w in zip(got, want))


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_fails_on_the_ladder(mutant, monkeypatch):
    D = A.case_data("uni_" + MUTANTS[mutant][0])
    clean = _value_ratio(O.forward(D["spec"], D["z"], D["th"], np.float32), (D["x"], D["ldj"]))
    r = _value_ratio(_mutated_forward(monkeypatch, mutant, D["spec"], D["z"], D["th"]), (D["x"], D["ldj"]))
    print(f"MUTANT {mutant} on the ladder chain: ratio {r:.3g} (the real activation: {clean:.3f})")
    assert clean <= HALF
    assert r > 1.0, f"{mutant} passes the value criterion on the ladder chain (ratio {r})"


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_passes_on_test_activations_chain(mutant, monkeypatch):
    """The chain and inputs of test_gpu_parity.py::test_activations: the gap."""
    act = MUTANTS[mutant][0]
    rng = np.random.default_rng(7)
    ch = dfa.FlowChain(dfa.CouplingLayer(5, [2, 4], hidden_dim=32, σ=act, rng=rng),
                       dfa.CouplingLayer(5, [1, 3, 5], hidden_dim=32, σ=act, rng=rng))
    z = rng.standard_normal((5, 300)).astype(np.float32)
    spec, th = ch.to_spec(), np.zeros((0, 300))
    want = O.forward(spec, z, th, np.float64)
    r = _value_ratio(_mutated_forward(monkeypatch, mutant, spec, z, th), want)
    print(f"MUTANT {mutant} on test_activations' chain: ratio {r:.3g}")
    assert r <= 1.0, f"{mutant} is caught by test_activations' chain already (ratio {r})"
