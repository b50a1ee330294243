"""GPU tests of df_train_logpdf_grad: per-sample ∂logpdf/∂x and ∂logpdf/∂θ against the fp64
analytic reference (tests/score_ref.py, pinned to finite differences in
tests/test_score_ref.py).

Criterion: the project's gradient criterion, helpers.close(g, ref, 1e-4, 2e-5), on gx and
on gθ separately; helpers.close at its defaults on lp.

Relu kinks: an f32 pre-activation within rounding of 0 may take the other branch of σ'
than the fp64 reference, which changes that one sample's gradient by O(1).  Samples whose
reference kink distance (smallest |pre-activation| over the relu Denses) is below 1e-5 are
dropped from the comparison; the dropped share is asserted under a cap the reference alone
meets (readme: 0 at B = 1 and 17, 0.5 % at 1000, 0.77 % at 70001, cap 2 %; cfg2: 1 of 17,
7.2 % at 1000, cap 10 %).  Smooth-activation chains drop nothing.
"""
import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib
from densityflows_amd.data import MetaData
from densityflows_amd.train import Adam, HIPTrainer, trainables
from helpers import close, spec_to_element
from oracle import flow_oracle as O
import score_ref as R
from test_gpu_train import (G_ATOL, G_RTOL, SPECS, _dev, _flat_oracle_grads, _gpu_grad, _inputs, _tensor_slices)

pytestmark = pytest.mark.gpu

KINK = 1e-5
PRE_ACTS = ["softplus", "swish", "logcosh", "softplus", "swish"]


def _spec(name):
    """(spec, d, n): the chains of tests/test_gpu_train.py with weights from default_rng(0);
    "pre": the construction of tests/test_score_ref.py with pre-activation σ'."""
    rng = np.random.default_rng(0)
    if name == "pre":
        return R.pre_spec(rng, PRE_ACTS, n=2), 5, 2
    make, d, n = SPECS[name]
    return make(rng), d, n


_REF = {}


def _case(name, B):
    """(spec, x, θ, reference) — computed once per (chain, B) and shared, never modified."""
    if (name, B) not in _REF:
        spec, d, n = _spec(name)
        x, th = _inputs(d, n, B)
        _REF[name, B] = (spec, x, th, R.logpdf_grad(spec, x, th))
    return _REF[name, B]


def _trainer(spec, given=True):
    tr = HIPTrainer(spec_to_element(spec).hip(), Adam())
    if given:
        tr.set_theta_input(_lib.DF_THETA_GIVEN)
    return tr


def _run(tr, x, th, cuda, lp=True, gx=True, gth=True):
    """df_train_logpdf_grad → numpy (lp (B,), gx (d, B), gθ (n, B)); None for a NULL output."""
    import torch

    d, B = x.shape
    n = th.shape[0]
    lpb = torch.full((B,), np.nan, dtype=torch.float32, device=cuda) if lp else None
    gxb = torch.full((B * d,), np.nan, dtype=torch.float32, device=cuda) if gx else None
    gtb = torch.full((B * n,), np.nan, dtype=torch.float32, device=cuda) if (gth and n) else None
    tr.logpdf_grad(_dev(x, cuda), _dev(th, cuda) if n else None, B, lpb, gxb, gtb)
    torch.cuda.synchronize()
    out = lambda b, rows: None if b is None else b.cpu().numpy().reshape(B, rows).T.copy()
    return (None if lpb is None else lpb.cpu().numpy().copy()), out(gxb, d), out(gtb, n)


def _check(got, ref, cap, what=""):
    lp, gx, gth = got
    rlp, rgx, rgth, kink = ref
    keep = kink >= KINK
    dropped = 1.0 - float(np.mean(keep))
    assert dropped <= cap, f"{what}: {dropped:.4f} of the samples within {KINK} of a relu kink (cap {cap})"
    ratios = {"lp": close(lp[keep], rlp[keep])[1], "gx": close(gx[:, keep], rgx[:, keep], G_RTOL, G_ATOL)[1]}
    if rgth.shape[0]:
        ratios["gth"] = close(gth[:, keep], rgth[:, keep], G_RTOL, G_ATOL)[1]
    print(f"{what}: dropped {dropped:.4f}, violation ratios {ratios}")
    assert max(ratios.values()) <= 1.0, f"{what}: violation ratios {ratios} (dropped {dropped:.4f})"


# readme at 70001: one past what makes a wave run its tile loop a second time.  A launch is
# at most 4 workgroups of 4 waves on each of the 256 CUs (the readme instances hold ≤ 126
# VGPRs: 4 waves per SIMD), every wave one 16-sample tile per pass: 16 · 4 · 1024 = 65536
# samples in the first pass, so sample 65536 + 17 <= 70001 is in a second one.
@pytest.mark.parametrize("name,B,cap", [("readme", 1, 0.0), ("readme", 17, 0.0), ("readme", 1000, 0.02),
                                        ("cfg2", 17, 0.10), ("cfg2", 1000, 0.10), ("mixed", 777, 0.0),
                                        ("pre", 33, 0.0), ("readme", 70001, 0.02)])
def test_parity(cuda, name, B, cap):
    spec, x, th, ref = _case(name, B)
    tr = _trainer(spec)
    _check(_run(tr, x, th, cuda), ref, cap, f"{name} B={B}")


@pytest.mark.parametrize("name,B,cap", [("readme", 1000, 0.02), ("cfg2", 17, 0.10)])
def test_parity_per_net_launches(cuda, monkeypatch, name, B, cap):
    """DF_SCORE_PER_NET=1 (read when the trainer is created): one launch per net, exp(-s)
    through the workspace, instead of one per RNVP layer — the form layers whose two nets
    differ in depth take."""
    monkeypatch.setenv("DF_SCORE_PER_NET", "1")
    spec, x, th, ref = _case(name, B)
    tr = _trainer(spec)
    _check(_run(tr, x, th, cuda), ref, cap, f"{name} B={B} per net")


def test_theta_conventions(cuda):
    """DF_THETA_GIVEN on pre-normalised θ against DF_THETA_RAW with bounds (one max == min row)."""
    spec, d, n = _spec("mixed")
    B = 777
    x, thn = _inputs(d, n, B)
    tmin = np.array([-1.5, 0.75], np.float32)
    tmax = np.array([2.5, 0.75], np.float32)
    thn[1, :] = 0.0                                   # normalize_input of a constant row
    raw = (thn * (tmax - tmin)[:, None] + tmin[:, None]).astype(np.float32)
    chain = spec_to_element(spec).hip()
    chain.set_theta_bounds(tmin, tmax)
    tr = HIPTrainer(chain, Adam())
    tr.set_theta_input(_lib.DF_THETA_GIVEN)
    lp_n, gx_n, gth_n = _run(tr, x, thn, cuda)
    tr.set_theta_input(_lib.DF_THETA_RAW)
    lp_r, gx_r, gth_r = _run(tr, x, raw, cuda)
    assert close(lp_r, lp_n)[0]
    assert close(gx_r, gx_n, G_RTOL, G_ATOL)[0]
    ok, r = close(gth_r[0], gth_n[0] / 4.0, G_RTOL, G_ATOL)
    assert ok, r
    assert np.any(gth_n[1] != 0)
    assert np.array_equal(gth_r[1].view(np.uint32), np.zeros(B, np.uint32))  # bitwise +0.0
    # and both are right
    ref = R.logpdf_grad(spec, x, raw, tmin, tmax)
    _check((lp_r, gx_r, gth_r), ref, 0.0, "mixed raw θ")


@pytest.mark.parametrize("name", ["readme", "cfg2"])
def test_null_outputs(cuda, name):
    """A NULL output is not written and leaves the others bitwise those of the full call
    (cfg2: n = 0, grad_theta is NULL throughout)."""
    spec, x, th, _ = _case(name, 1000)
    tr = _trainer(spec)
    full = _run(tr, x, th, cuda)
    assert (full[2] is None) == (th.shape[0] == 0)
    for drop in range(3):
        flags = [k != drop for k in range(3)]
        got = _run(tr, x, th, cuda, *flags)
        for k in range(3):
            if k == drop or full[k] is None:
                assert got[k] is None
            else:
                np.testing.assert_array_equal(got[k], full[k])


def test_reproducible_and_isolated(cuda):
    spec, x, th, _ = _case("readme", 1000)
    tr, twin = _trainer(spec), _trainer(spec)
    a = _run(tr, x, th, cuda)
    b = _run(tr, x, th, cuda)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    g0, lp0 = _gpu_grad(tr, x, th, cuda)
    c = _run(tr, x, th, cuda)
    np.testing.assert_array_equal(c[1], a[1])
    np.testing.assert_array_equal(tr.grad().detach().cpu().numpy(), g0)
    tr.apply()
    g1, lp1 = _gpu_grad(twin, x, th, cuda)
    twin.apply()
    np.testing.assert_array_equal(g1, g0)
    assert lp1 == lp0
    np.testing.assert_array_equal(tr.get_params(), twin.get_params())


def _load_flat(spec, flat):
    """Write a flat Flux.trainables vector into the spec's Dense layers."""
    o = 0
    for L in O._flat_layers(spec):
        for net in ("s_net", "t_net"):
            for D in L.get(net, []) if L["kind"] != "norm" else []:
                k = D["W"].size
                D["W"] = flat[o:o + k].reshape(D["W"].shape, order="F").copy()
                o += k
                if D.get("b") is not None:
                    D["b"] = flat[o:o + D["b"].size].copy()
                    o += D["b"].size
    assert o == flat.shape[0]


def test_follows_the_weights(cuda):
    """After Adam steps the call evaluates the trainer's current parameters."""
    spec, d, n = _spec("readme")
    B = 1000
    x, th = _inputs(d, n, B)
    tr = _trainer(spec)
    p0 = tr.get_params()
    for _ in range(3):
        tr.step(_dev(x, cuda), _dev(th, cuda), B)
    p = tr.get_params()
    assert np.max(np.abs(p - p0)) > 1e-4
    got = _run(tr, x, th, cuda)
    _load_flat(spec, p)
    np.testing.assert_array_equal(trainables(spec_to_element(spec)), p)
    _check(got, R.logpdf_grad(spec, x, th), 0.02, "readme after 3 steps")
    stale = _case("readme", B)[3]
    assert not close(got[1], stale[1], G_RTOL, G_ATOL)[0]


def test_unsupported_class_leaves_trainer_usable(cuda):
    spec, d, n = _spec("wide")
    B = 64
    x, th = _inputs(d, n, B)
    tr = _trainer(spec, given=False)
    with pytest.raises(_lib.UnsupportedError, match="hidden width > 64"):
        _run(tr, x, th, cuda)
    g, lpsum = _gpu_grad(tr, x, th, cuda)
    loss, ref = O.nll_and_grad(spec, x, th)
    ref = _flat_oracle_grads(spec, ref)
    assert abs(-lpsum / B - loss) <= 1e-5 * max(1.0, abs(loss))
    for sl in _tensor_slices(spec):
        ok, r = close(g[sl], ref[sl], G_RTOL, G_ATOL)
        assert ok, r


def test_high_level_api(cuda):
    spec, d, n = _spec("readme")
    tmin, tmax = np.array([-1.0], np.float32), np.array([3.0], np.float32)
    flow = dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, tmin, tmax))
    rng = np.random.default_rng(1)
    x = rng.standard_normal((5, 2, 5, 7)).astype(np.float32)
    t1 = 1.25
    lp, gx, gth = dfa.logpdf_grad(flow, x, (t1,))
    assert all(isinstance(a, np.ndarray) for a in (lp, gx, gth))
    assert lp.shape == (2, 5, 7) and gx.shape == (5, 2, 5, 7) and gth.shape == (1, 2, 5, 7)
    xf = x.reshape(5, 70, order="F")
    lp2, gx2, gth2 = dfa.logpdf_grad(flow, xf, np.full((1, 70), t1, np.float32))
    assert lp2.shape == (70,) and gx2.shape == (5, 70) and gth2.shape == (1, 70)
    np.testing.assert_array_equal(lp.reshape(70, order="F"), lp2)
    np.testing.assert_array_equal(gx.reshape(5, 70, order="F"), gx2)
    np.testing.assert_array_equal(gth.reshape(1, 70, order="F"), gth2)
    # the flow's logpdf, and the reference in the raw θ
    assert close(lp2, dfa.logpdf(flow, xf, np.full((1, 70), t1, np.float32)))[0]
    ref = R.logpdf_grad(spec, xf, np.full((1, 70), t1), tmin, tmax)
    _check((lp2, gx2, gth2), ref, 0.02, "flow-level")
    # a TrainState's trainer serves the call, and df_chain_set_weights is not left blocked
    state = dfa.setup(Adam(), flow)
    lp3, gx3, gth3 = dfa.logpdf_grad(flow, xf, np.full((1, 70), t1, np.float32), state=state)
    np.testing.assert_array_equal(gx3, gx2)
    np.testing.assert_array_equal(gth3, gth2)
    del state
    flow.hip().set_weights(flow.model.layers)
