"""CPU checks of the input-gradient reference (tests/score_ref.py) and of the host side
of df_train_logpdf_grad.

The reference is pinned to central differences of the oracle's flow_logpdf; the GPU
tests (tests/test_gpu_score.py) then compare the kernels against it.
"""
import ctypes as C

import numpy as np
import pytest

from densityflows_amd import _lib
from oracle import flow_oracle as O
import score_ref as R

D, N, B = 5, 2, 37


def _case(act):
    spec = R.pre_spec(np.random.default_rng(0), act, n=N)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((D, B))
    th = rng.random((N, B))
    return spec, x, th


def _central(f, v, h=1e-6):
    """Central differences of the per-sample function f (→ (B,)) in every row of v."""
    g = np.zeros_like(v)
    for i in range(v.shape[0]):
        e = np.zeros_like(v)
        e[i, :] = h
        g[i] = (f(v + e) - f(v - e)) / (2 * h)
    return g


@pytest.mark.parametrize("act", ["tanh", "softplus"])
def test_reference_equals_central_differences(act):
    spec, x, th = _case(act)
    lp, gx, gth, kink = R.logpdf_grad(spec, x, th)
    assert lp.shape == (B,) and gx.shape == (D, B) and gth.shape == (N, B) and kink.shape == (B,)
    np.testing.assert_allclose(lp, O.flow_logpdf(spec, x, th), rtol=0, atol=1e-12)
    fx = _central(lambda v: O.flow_logpdf(spec, v, th), x)
    ft = _central(lambda v: O.flow_logpdf(spec, x, v), th)
    scale = max(np.max(np.abs(gx)), np.max(np.abs(gth)))
    ex, et = np.max(np.abs(gx - fx)), np.max(np.abs(gth - ft))
    print(f"{act}: max|gx - fd| = {ex:.3g}, max|gθ - fd| = {et:.3g}, max|grad| = {scale:.3g}")
    assert ex <= 1e-6 * scale and et <= 1e-6 * scale
    assert np.all(np.isinf(kink))  # smooth activations have no kink


@pytest.mark.parametrize("act", ["tanh", "softplus"])
def test_raw_theta_rule(act):
    """gθ_raw = gθ_n / (max − min), exactly 0 in a row with max == min."""
    spec, x, thn = _case(act)
    tmin = np.array([-1.5, 0.75])
    tmax = np.array([2.5, 0.75])           # row 1: max == min → normalised to 0
    thn[1, :] = 0.0
    raw = thn * (tmax - tmin)[:, None] + tmin[:, None]
    lp_n, gx_n, gth_n, _ = R.logpdf_grad(spec, x, thn)
    lp_r, gx_r, gth_r, _ = R.logpdf_grad(spec, x, raw, tmin, tmax)
    np.testing.assert_allclose(lp_r, lp_n, rtol=0, atol=1e-12)
    np.testing.assert_allclose(gx_r, gx_n, rtol=0, atol=1e-12)
    np.testing.assert_allclose(gth_r[0], gth_n[0] / 4.0, rtol=1e-12, atol=0)
    assert np.any(gth_n[1] != 0)
    assert np.all(gth_r[1] == 0.0)
    # and it is the derivative in the raw θ
    ft = _central(lambda v: O.flow_logpdf(spec, x, O.normalize_input(v, tmin, tmax, np.float64)), raw)
    assert np.max(np.abs(gth_r - ft)) <= 1e-6 * max(np.max(np.abs(gx_n)), np.max(np.abs(gth_n)))


def test_relu_kink_distance():
    spec = R.pre_spec(np.random.default_rng(0), "relu", n=N)
    _, x, th = _case("relu")
    *_, kink = R.logpdf_grad(spec, x, th)
    assert np.all(np.isfinite(kink)) and np.all(kink >= 0)
    # it is the smallest |pre-activation|: recompute it for the last layer inverted first
    L = O._flat_layers(spec)[-2]
    u, _ = O.norm_backward(O._flat_layers(spec)[-1], x, th, np.float64)
    _, cache = O._mlp_forward_cache(L["t_net"], O._conditioner_input(L, u, th, np.float64), np.float64)
    assert np.all(kink <= np.min(np.abs(cache[0][1]), axis=0))


def test_host_entry_point():
    """The library exports df_train_logpdf_grad, refuses a null trainer without touching
    a device, and the header, the library and the Python binding agree on ABI 5."""
    lib = _lib.load()
    assert hasattr(lib, "df_train_logpdf_grad")
    assert "df_train_logpdf_grad" in _lib.SIGNATURES
    x = np.zeros(5, np.float32)
    rc = lib.df_train_logpdf_grad(None, x.ctypes.data_as(C.c_void_p), None, None, None, None, C.c_int64(1), None)
    assert rc == _lib.DF_ERR_INVALID
    assert b"null trainer" in lib.df_last_error()
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION
