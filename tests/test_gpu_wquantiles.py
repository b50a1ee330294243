"""GPU tests of the weighted quantile calls (df_wquant.hip): df_draw_weight_scale,
df_draw_weighted_quantiles and their Python mirrors.

Everything past the quantisation of the weights is integer arithmetic: every comparison with the
host reference (tests/wquantile_ref.py: Python ints and uint64 numpy) is ``==`` on bytes, and no
tolerance appears anywhere.  Every output buffer is pre-filled with a sentinel the call cannot
produce and followed by GUARD words that must survive.

The kernels map a wave to a point up to N = 256 and a workgroup above; above 16 probabilities the
selection takes a workgroup per point at every N.  The shapes stand on both sides of 256, take a
second trip (4100) and hold more points than one workgroup's four teams (257).  d = 32 and 61 walk
several groups of dimensions.

No test states a statistical claim: the models are untrained.  One point's intervals are printed.
"""
import ctypes as C

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib
from densityflows_amd.data import MetaData
from helpers import spec_to_element
import quantile_ref as Q
import wquantile_ref as W
from test_gpu_moments import _bounds
from test_gpu_score import _spec
from test_gpu_train import _inputs

pytestmark = pytest.mark.gpu

GUARD = 8
ONE = 1 << 32
FILL_BITS = 0x7FEDCBA9          # a NaN payload no draw of these tests holds
FILL_SCALE = -0x123456789       # no exponent and no sum is this

SHAPES = [(1, 4), (3, 12), (17, 64), (5, 68), (3, 256), (3, 260), (257, 4), (2, 4100)]
DIMS = [1, 5, 8, 32, 61]
PROBS = {
    1: [0.5],
    6: [0.0, 0.16, 0.5, 0.5, 0.84, 1.0],
    12: list(np.linspace(0.02, 0.98, 12)),
    32: [0.0, 1.0, 0.5, 0.5] + list(np.linspace(0.01, 0.99, 28)),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scale(cuda, w):
    """One df_draw_weight_scale call on numpy weights (M, N) → (M, 2) int64."""
    import torch

    M, N = w.shape
    wb = torch.from_numpy(np.ascontiguousarray(w)).to(cuda)
    sc = torch.full((2 * M + GUARD,), FILL_SCALE, dtype=torch.int64, device=cuda)
    dfa.hip.run_draw_weight_scale(wb, M, N, sc)
    torch.cuda.synchronize()
    v = sc.cpu().numpy()
    assert np.all(v[2 * M:] == FILL_SCALE), "scale_out written past 2 · n_points"
    assert np.all(v[:2 * M] != FILL_SCALE), "scale_out not fully written"
    return v[:2 * M].reshape(M, 2).copy()


def _wq(cuda, x, w, nums):
    """One df_draw_weighted_quantiles call on numpy draws (M, N, d) and weights (M, N) →
    (bits (M, d, P) uint32, scale (M, 2) int64)."""
    import torch

    M, N, d = x.shape
    P = len(nums)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    wb = torch.from_numpy(np.ascontiguousarray(w)).to(cuda)
    out = torch.from_numpy(np.full(M * d * P + GUARD, FILL_BITS, np.uint32).view(np.float32)).to(cuda)
    sc = torch.full((2 * M + GUARD,), FILL_SCALE, dtype=torch.int64, device=cuda)
    dfa.hip.run_draw_weighted_quantiles(xs, wb, d, M, N, nums, out, sc)
    torch.cuda.synchronize()
    v = out.cpu().numpy().view(np.uint32)
    s = sc.cpu().numpy()
    assert np.all(v[M * d * P:] == FILL_BITS), "quant_out written past n_points · d · n_probs"
    assert np.all(v[:M * d * P] != FILL_BITS), "quant_out not fully written"
    assert np.all(s[2 * M:] == FILL_SCALE) and np.all(s[:2 * M] != FILL_SCALE)
    return v[:M * d * P].reshape(M, d, P).copy(), s[:2 * M].reshape(M, 2).copy()


def _draws(M, N, d, seed):
    rng = np.random.default_rng(seed)
    return W.plant_draws(rng.standard_normal((M, N, d)).astype(np.float32), rng), rng


def _check_scale(s, w):
    e, T, _ = W.scales(w)
    np.testing.assert_array_equal(s[:, 0], e)
    np.testing.assert_array_equal(s[:, 1], T)


# ---------------------------------------------------------------------------
# 1. the scale and the quantiles against the integer reference, every weight pattern
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N", SHAPES + [(2, 65540)])
def test_weight_scale_exact(cuda, M, N):
    rng = np.random.default_rng(N + M)
    for name, w in W.weight_patterns(M, N, rng).items():
        _check_scale(_scale(cuda, w), w)
    w = W.weight_patterns(M, N, rng)["hostile"]
    e, T = dfa.weight_scale(w)
    _check_scale(np.stack([e, T], axis=1), w)


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_weighted_quantiles_exact(cuda, d, M, N):
    x, rng = _draws(M, N, d, 1000 * d + N + M)
    sets = list(PROBS)
    for j, (name, w) in enumerate(W.weight_patterns(M, N, rng).items()):
        # every pattern at 6 probabilities, and one of the other counts in turn (all of them at unit weights)
        for P in [6] + (sets if name == "unit" else [sets[(j + d) % len(sets)]]):
            nums = W.numerators(PROBS[P])
            got, s = _wq(cuda, x, w, nums)
            _check_scale(s, w)
            np.testing.assert_array_equal(got, _bits(W.quantiles(x, w, nums)), err_msg=f"{name}, {P} probabilities")
        if name == "hostile" and M > 1:                    # the empty point among others
            assert (s[M // 2] == 0).all() and (got[M // 2] == W.NAN_BITS).all()


@pytest.mark.parametrize("d,M,N", [(3, 2, 65540), (1, 1, 1 << 20)])
def test_many_draws(cuda, d, M, N):
    rng = np.random.default_rng(N)
    x = rng.standard_normal((M, N, d)).astype(np.float32)
    x[:, ::97] = np.float32(0.5)                            # ties
    w = np.exp(3.0 * rng.standard_normal((M, N))).astype(np.float32)
    w[:, ::5] = 0.0
    nums = W.numerators(PROBS[6])
    got, s = _wq(cuda, x, w, nums)
    _check_scale(s, w)
    np.testing.assert_array_equal(got, _bits(W.quantiles(x, w, nums)))


# ---------------------------------------------------------------------------
# 2. unit weights: order statistic r of df_order_statistics, on the device
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,d", [(4, 5), (64, 8), (256, 5), (1024, 5), (4096, 33)])
def test_unit_weights_are_order_statistics(cuda, N, d):
    import torch

    M = 3
    x, rng = _draws(M, N, d, N)
    orders = sorted({0, 1, N // 4, N // 2, N - 2, N - 1})
    nums = [(r + 1) * ONE // N for r in orders]
    got, s = _wq(cuda, x, np.ones((M, N), np.float32), nums)
    assert (s[:, 0] == 1).all() and (s[:, 1] == N << 31).all()
    xs = torch.from_numpy(x).to(cuda)
    ref = torch.empty((M, d, len(orders)), dtype=torch.float32, device=cuda)
    dfa.hip.run_order_statistics(xs, d, M, N, orders, ref)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, _bits(ref.cpu().numpy()))
    np.testing.assert_array_equal(got, _bits(Q.order_stats(x, orders)))


# ---------------------------------------------------------------------------
# 3. independence of the other points; two calls
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,P", [(12, 6), (12, 32), (260, 6)])
def test_independent_of_the_other_points(cuda, N, P):
    M, d = 257, 5
    x, rng = _draws(M, N, d, 31 * N + P)
    w = W.weight_patterns(M, N, rng)["lognormal3"]
    nums = W.numerators(PROBS[P])
    all_, s = _wq(cuda, x, w, nums)
    again, s2 = _wq(cuda, x, w, nums)
    np.testing.assert_array_equal(all_, again)
    np.testing.assert_array_equal(s, s2)
    for i in (0, 130, 256):
        one, s1 = _wq(cuda, x[i:i + 1], w[i:i + 1], nums)
        np.testing.assert_array_equal(one[0], all_[i])
        np.testing.assert_array_equal(s1[0], s[i])


# ---------------------------------------------------------------------------
# 4. the argument rules on device arrays; an empty call writes nothing
# ---------------------------------------------------------------------------

def test_argument_rules_and_empty_call(cuda):
    import torch

    lib = _lib.load()
    M, N, d = 2, 8, 3
    xs = torch.zeros((M, N, d), dtype=torch.float32, device=cuda)
    w = torch.ones((M, N), dtype=torch.float32, device=cuda)
    out = torch.from_numpy(np.full(M * d * 3, FILL_BITS, np.uint32).view(np.float32)).to(cuda)
    sc = torch.full((2 * M,), FILL_SCALE, dtype=torch.int64, device=cuda)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    null = C.c_void_p(0)
    nums = (C.c_uint64 * 3)(0, ONE // 2, ONE)

    def call(xs=p(xs), w=p(w), d=d, n_points=M, n_draws=N, nums=nums, n_probs=3, out=p(out), sc=p(sc)):
        return lib.df_draw_weighted_quantiles(xs, w, d, n_points, n_draws, nums, n_probs, out, sc, null)

    msg = lambda: lib.df_last_error().decode()
    assert call(d=65) == _lib.DF_ERR_INVALID and "1 .. 64" in msg()
    assert call(d=65, n_points=-1) == _lib.DF_ERR_INVALID
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, xs=null) == _lib.DF_ERR_INVALID and "multiple of 4" in msg()
    assert call(xs=null, w=p(w, 4)) == _lib.DF_ERR_INVALID and "null" in msg()
    assert call(w=p(w, 4), n_probs=33) == _lib.DF_ERR_INVALID and "16-byte" in msg()
    assert call(n_probs=33, nums=(C.c_uint64 * 3)(ONE + 1, 0, 0)) == _lib.DF_ERR_UNSUPPORTED and "n_probs" in msg()
    assert call(nums=(C.c_uint64 * 3)(0, 0, ONE + 1)) == _lib.DF_ERR_INVALID and "nums[2]" in msg()
    assert lib.df_draw_weight_scale(p(w), -1, N, p(sc), null) == _lib.DF_ERR_SHAPE
    assert lib.df_draw_weight_scale(p(w, 4), M, N, p(sc), null) == _lib.DF_ERR_INVALID
    # an empty call: DF_OK, the poisoned outputs keep their bytes
    assert call(n_points=0) == _lib.DF_OK
    assert lib.df_draw_weight_scale(p(w), 0, N, p(sc), null) == _lib.DF_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == FILL_BITS).all() and (sc.cpu().numpy() == FILL_SCALE).all()
    with pytest.raises(_lib.ArgumentError, match=r"nums\[0\]"):
        dfa.hip.run_draw_weighted_quantiles(xs, w, d, M, N, [ONE + 1], out, sc)
    assert dfa.weighted_quantiles(np.zeros((0, 8, 3), np.float32), np.zeros((0, 8), np.float32)).shape == (0, 3, 3)


# ---------------------------------------------------------------------------
# 5. the Python mirrors and the chain on a flow
# ---------------------------------------------------------------------------

def test_python_mirrors(cuda):
    import torch

    M, N, d = 5, 68, 5
    x, rng = _draws(M, N, d, 5)
    w = W.weight_patterns(M, N, rng)["lognormal3"]
    probs = (0.16, 0.5, 0.84)
    ref = _bits(W.quantiles(x, w, W.numerators(probs)))
    got = dfa.weighted_quantiles(x, w)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (M, d, 3)
    np.testing.assert_array_equal(_bits(got), ref)
    gt = dfa.weighted_quantiles(torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda), probs)
    assert isinstance(gt, torch.Tensor) and gt.device.type == "cuda"
    np.testing.assert_array_equal(_bits(gt.cpu().numpy()), ref)
    lo, med, hi = dfa.weighted_credible_intervals(x, w, level=0.68)
    for k, v in enumerate((lo, med, hi)):
        np.testing.assert_array_equal(_bits(v), ref[:, :, k])
    iw = dfa.importance_weights(np.log(w))
    np.testing.assert_array_equal(_bits(dfa.weighted_quantiles(x, iw)), _bits(W.quantiles(x, iw.w, W.numerators(probs))))


def _flow(name):
    spec, d, n = _spec(name)
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, *_bounds(n)))


@pytest.mark.parametrize("name,M,N", [("readme", 8, 64), ("cfg2", 2, 260)])
def test_importance_posterior_quantiles_on_a_flow(cuda, name, M, N):
    import torch

    flow = _flow(name)
    d, n = flow.d, flow.n
    seed, offset = 515, 4
    th = _inputs(d, n, M)[1] if n else None
    kw = dict(n_draws=N, dims=(M,), seed=seed, offset=offset)
    qt, lqt = dfa.posterior_draws(flow, th, as_tensor=True, **kw)
    calls = []

    def log_target(draws, theta):                # log q plus a Gaussian: the weights come from the Gaussian
        calls.append(tuple(draws.shape))
        assert isinstance(draws, torch.Tensor) and draws.device.type == "cuda"
        return lqt - 0.5 * ((draws - 0.25) ** 2).sum(dim=-1)

    probs = (0.025, 0.16, 0.5, 0.84, 0.975)
    got, iw = dfa.importance_posterior_quantiles(flow, th, log_target, probs=probs, **kw)
    assert calls == [(M, N, d)]
    assert isinstance(got, np.ndarray) and got.shape == (M, d, 5) and got.dtype == np.float32
    # the three chained calls made by hand, bit for bit
    iw2 = dfa.importance_weights(log_target(qt, th), lqt)
    by_hand = dfa.weighted_quantiles(qt, iw2, probs).cpu().numpy()
    np.testing.assert_array_equal(_bits(iw.w.cpu().numpy()), _bits(iw2.w.cpu().numpy()))
    np.testing.assert_array_equal(_bits(got), _bits(by_hand))
    # and the reference on the device's own draws and weights
    x, w = qt.cpu().numpy(), iw.w.cpu().numpy()
    np.testing.assert_array_equal(_bits(got), _bits(W.quantiles(x, w, W.numerators(probs))))
    (lo, med, hi), _ = dfa.importance_credible_intervals(flow, th, log_target, level=0.68, **kw)
    np.testing.assert_array_equal(_bits(lo), _bits(got[:, :, 1]))
    np.testing.assert_array_equal(_bits(med), _bits(got[:, :, 2]))
    np.testing.assert_array_equal(_bits(hi), _bits(got[:, :, 3]))
    plain = dfa.order_statistics(x, [int(0.16 * (N - 1)), N // 2, int(0.84 * (N - 1))])
    res = dfa.order_statistics(dfa.resample(x, w, seed=seed), [int(0.16 * (N - 1)), N // 2, int(0.84 * (N - 1))])
    print(f"{name} (untrained), point 0, dimension 0: weighted {lo[0, 0]:.4f} {med[0, 0]:.4f} {hi[0, 0]:.4f}, "
          f"unweighted {plain[0, 0]}, resampled {res[0, 0]}, ESS {iw.ess[0]:.1f} of {N}")
