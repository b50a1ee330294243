"""Host side of the order-statistics calls (df_quant.hip), on CPU: df_order_statistics and
df_flow_point_quantiles are declared, bound and exported at ABI 5; their argument errors come
back before any device work, each with a message naming the rule; the Python wrappers refuse bad
arguments before the library is touched; the reference functions of tests/quantile_ref.py agree
with brute-force loops and with numpy; quantile_orders is numpy's linear rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
from densityflows_amd.data import MetaData
from helpers import spec_to_element
from train_edge_cases import SPECS
import quantile_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calls_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densityflows_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, count in (("df_order_statistics", 8), ("df_flow_point_quantiles", 15)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == count
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == count
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+DF_QUANT_MAX_ORDERS\s+32\b", src)
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", src)
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION
    assert hasattr(dfa.hip.HIPChain, "run_point_quantiles") and hasattr(dfa.hip.HIPChain, "run_order_statistics")
    assert hasattr(dfa.hip, "run_order_statistics")
    for name in ("quantile_orders", "order_statistics", "posterior_quantiles", "credible_intervals"):
        assert name in flows.__all__ and hasattr(dfa, name)
    assert dfa.QUANT_MAX_ORDERS == 32


def _orders(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def _message(lib):
    return lib.df_last_error().decode("utf-8")


def test_order_statistics_argument_errors_before_device_work():
    """No device exists here: every status below is returned before anything is launched."""
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    base = (C.addressof(buf) + 15) & ~15
    xs, out, null = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(0)

    def call(xs=xs, d=5, n_points=4, n_draws=8, orders=_orders(0, 7), n_orders=2, out=out):
        return lib.df_order_statistics(xs, d, n_points, n_draws, orders, n_orders, out, null)

    for bad in (0, -1, 65):
        assert call(d=bad) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(lib), bad
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message(lib)
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib), bad
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib)
    assert call(xs=null) == _lib.DF_ERR_INVALID and "null" in _message(lib)
    assert call(out=null) == _lib.DF_ERR_INVALID and "null" in _message(lib)
    for off in (4, 8, 12):
        assert call(xs=C.c_void_p(base + off)) == _lib.DF_ERR_INVALID and "16-byte" in _message(lib), off
    assert call(orders=None) == _lib.DF_ERR_INVALID and "null orders" in _message(lib)
    for bad in (0, -1, 33):
        assert call(orders=_orders(*([0] * 33)), n_orders=bad) == _lib.DF_ERR_UNSUPPORTED, bad
        assert "n_orders" in _message(lib), bad
    assert call(orders=_orders(0, 3, 8), n_orders=3) == _lib.DF_ERR_INVALID and "orders[2]" in _message(lib)
    assert call(orders=_orders(-1, 3), n_orders=2) == _lib.DF_ERR_INVALID and "orders[0]" in _message(lib)
    # the same rules hold for an empty call
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, d=0) == _lib.DF_ERR_INVALID
    assert call(n_points=0, xs=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_orders=33) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, orders=_orders(8), n_orders=1) == _lib.DF_ERR_INVALID and "orders[0]" in _message(lib)
    # an empty call with sound arguments launches nothing
    assert call(n_points=0) == _lib.DF_OK
    assert call(n_points=0, orders=_orders(*range(8), *range(8), *range(8), *range(8)), n_orders=32) == _lib.DF_OK
    with pytest.raises(_lib.ArgumentError, match=r"orders\[1\]"):
        _lib.check(call(orders=_orders(0, 9), n_orders=2))
    with pytest.raises(_lib.UnsupportedError, match="n_orders"):
        _lib.check(call(n_orders=33))
    with pytest.raises(_lib.DimensionMismatch):
        _lib.check(call(n_points=-3))


def test_point_quantiles_argument_errors_before_device_work():
    """The rules of df_flow_point_stats in its order and with its messages, then the outputs, then
    the orders: each returned by a check that stands before the first use of the handle (a
    non-null handle is a buffer that is never read)."""
    lib = _lib.load()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    null = C.c_void_p(0)
    out = C.c_void_p(C.addressof(C.create_string_buffer(8 * 16)))
    u = C.c_uint64

    def call(chain=fake, x=out, n_points=4, n_draws=8, chunk=0, orders=_orders(0, 7), n_orders=2, quant=out, rank=out,
             sums=out, draws=null):
        return lib.df_flow_point_quantiles(chain, x, null, n_points, n_draws, chunk, u(1), u(0), orders, n_orders,
                                           quant, rank, sums, draws, null)

    assert call(chain=null) == _lib.DF_ERR_INVALID and "null chain" in _message(lib)
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message(lib)
    assert call(chunk=-1) == _lib.DF_ERR_SHAPE and "chunk" in _message(lib)
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID, bad
        assert "multiple of 4" in _message(lib) and "Philox" in _message(lib), bad
    assert call(chunk=(1 << 24) + 1) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib) and "chunk" in _message(lib)
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib) and "n_draws" in _message(lib)
    assert call(quant=null, rank=null, sums=null) == _lib.DF_ERR_INVALID and "no output" in _message(lib)
    assert call(x=null) == _lib.DF_ERR_INVALID and "rank_out needs" in _message(lib)
    assert call(orders=None) == _lib.DF_ERR_INVALID and "null orders" in _message(lib)
    for bad in (0, -1, 33):
        assert call(orders=_orders(*([0] * 33)), n_orders=bad) == _lib.DF_ERR_UNSUPPORTED and "n_orders" in _message(lib)
    assert call(orders=_orders(0, 8), n_orders=2) == _lib.DF_ERR_INVALID and "orders[1]" in _message(lib)
    assert call(orders=_orders(-2, 1), n_orders=2) == _lib.DF_ERR_INVALID and "orders[0]" in _message(lib)
    # the order: the point count before n_draws, n_draws before the outputs, the outputs before the orders
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, quant=null, rank=null, sums=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib)
    assert call(quant=null, rank=null, sums=null, n_orders=33) == _lib.DF_ERR_INVALID and "no output" in _message(lib)
    assert call(x=null, n_orders=33) == _lib.DF_ERR_INVALID and "rank_out needs" in _message(lib)
    # the same rules hold for an empty call
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, quant=null, rank=null, sums=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, x=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_orders=33) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, orders=_orders(8), n_orders=1) == _lib.DF_ERR_INVALID
    # an empty call with sound arguments runs nothing: the fake handle is never read
    assert call(n_points=0) == _lib.DF_OK
    assert call(n_points=0, x=null, rank=null, sums=null) == _lib.DF_OK                     # quantiles alone
    # without quant_out the orders are not looked at
    assert call(n_points=0, quant=null, orders=None, n_orders=0) == _lib.DF_OK
    assert call(n_points=0, quant=null, orders=_orders(99), n_orders=77) == _lib.DF_OK
    assert call(n_points=0, x=null, quant=null, rank=null, sums=null, draws=out) == _lib.DF_OK
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        _lib.check(call(n_draws=6))
    with pytest.raises(_lib.UnsupportedError):
        _lib.check(call(chunk=(1 << 24) + 1))


def _flow(name="readme"):
    make, d, n = SPECS[name]
    spec = make(np.random.default_rng(0))
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, np.full(n, -1.0, np.float32),
                                                            np.full(n, 3.0, np.float32)))


def test_python_argument_errors(monkeypatch):
    """Raised before the library is touched: Flow.hip, _lib.load and the module-level order
    statistics call (the only ways to it) are never reached."""
    flow = _flow()

    def no_device(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(dfa.Flow, "hip", no_device)
    monkeypatch.setattr(dfa.hip, "run_order_statistics", no_device)
    x = np.zeros((5, 3, 2), np.float32)
    th = np.ones((1, 3, 2), np.float32)
    for fn in (lambda t, **k: dfa.posterior_quantiles(flow, t, x=x, seed=1, **k),
               lambda t, **k: dfa.posterior_quantiles(flow, t, x=x, seed=1, return_stats=True, **k),
               lambda t, **k: dfa.credible_intervals(flow, t, x=x, seed=1, **k)):
        for bad in ((1.0, 2.0), (), None, np.ones((1, 3), np.float32), np.ones((2, 3, 2), np.float32)):
            with pytest.raises(AssertionError, match="dimensions θ"):
                fn(bad)
        for bad in (0, -4, 6, 1023):
            with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
                fn(th, n_draws=bad)
        with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
            fn(th, chunk=(1 << 24) + 1)
        with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
            fn(th, n_draws=(1 << 24) + 4)
        with pytest.raises(_lib.DimensionMismatch, match="chunk"):
            fn(th, chunk=-4)
        # sound arguments reach the library
        with pytest.raises(AssertionError, match="the library was touched"):
            fn(th, n_draws=8)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(5, dims"):
        dfa.posterior_quantiles(flow, th, x=np.zeros((4, 3, 2), np.float32), seed=1)
    with pytest.raises(_lib.ArgumentError, match="dims="):
        dfa.posterior_quantiles(flow, (1.25,), seed=1)
    with pytest.raises(AssertionError, match="the library was touched"):
        dfa.posterior_quantiles(flow, (1.25,), n_draws=8, dims=(3, 2), seed=1)
    # the probabilities
    for bad in ((0.5, 1.5), (-0.1,), (np.nan,), ()):
        with pytest.raises(_lib.ArgumentError, match="probabilit"):
            dfa.posterior_quantiles(flow, th, probs=bad, seed=1)
    with pytest.raises(_lib.ArgumentError, match="at most 32"):
        dfa.posterior_quantiles(flow, th, probs=np.linspace(0.01, 0.99, 17), n_draws=4096, seed=1)
    for bad in (0.0, 1.0, -0.5, 1.5, np.nan):
        with pytest.raises(_lib.ArgumentError, match="level"):
            dfa.credible_intervals(flow, th, level=bad, seed=1)
    # order_statistics
    q = np.zeros((3, 8, 5), np.float32)
    with pytest.raises(_lib.ArgumentError, match="Float32"):
        dfa.order_statistics(q.astype(np.float64), [0])
    with pytest.raises(_lib.DimensionMismatch, match=r"\(M, N, d\)"):
        dfa.order_statistics(q[0], [0])
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        dfa.order_statistics(q[:, :6], [0])
    with pytest.raises(_lib.ArgumentError, match="1 .. 64"):
        dfa.order_statistics(np.zeros((1, 8, 65), np.float32), [0])
    for bad in ([], [8], [-1, 2], [0.5]):
        with pytest.raises(_lib.ArgumentError, match="orders"):
            dfa.order_statistics(q, bad)
    with pytest.raises(_lib.UnsupportedError, match="at most 32"):
        dfa.order_statistics(q, [0] * 33)


def test_key_order():
    """The key sort reproduces np.sort on finite values and infinities, puts −NaN first and +NaN
    last and −0 below +0, and the inverse returns every value's own bits."""
    rng = np.random.default_rng(4)
    v = np.concatenate([rng.standard_normal(500).astype(np.float32) * 1e3,
                        rng.standard_normal(50).astype(np.float32) * np.float32(1e-42),       # denormals
                        np.array([0.0, -0.0, np.inf, -np.inf, 3.4e38, -3.4e38, 1e-45, -1e-45], np.float32)])
    k = Q.keys(v)
    assert k.dtype == np.uint32
    np.testing.assert_array_equal(Q.bits(Q.values(k)), Q.bits(v))
    fin = v[np.argsort(k, kind="stable")]
    np.testing.assert_array_equal(fin, np.sort(v))
    z = fin[fin == 0]
    assert np.signbit(z[0]) and not np.signbit(z[-1])
    # brute force: key order is the order of the values wherever they differ
    for a in range(0, v.size, 7):
        for b in range(0, v.size, 11):
            if v[a] < v[b]:
                assert k[a] < k[b]
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    w = np.concatenate([v, nan])
    s = Q.values(np.sort(Q.keys(w)))
    assert Q.bits(s[0]) == 0xFFFFFFFF and Q.bits(s[1]) == 0xFFC00000            # −NaNs, the larger payload first
    assert Q.bits(s[-1]) == 0x7FC00000 and Q.bits(s[-2]) == 0x7F800001          # +NaNs last
    assert s[2] == -np.inf and s[-3] == np.inf


def test_order_stats_reference():
    rng = np.random.default_rng(5)
    M, N, d = 3, 12, 4
    q = rng.standard_normal((M, N, d)).astype(np.float32)
    q[0, :5, 1] = 0.25                                   # duplicates
    q[1, :3, 2] = [0.0, -0.0, 0.0]
    q[2, 4, 0] = np.nan
    orders = [0, 11, 5, 6, 5]
    ref = Q.order_stats(q, orders)
    assert ref.shape == (M, d, 5) and ref.dtype == np.float32
    for i in range(M):
        for k in range(d):
            col = [int(Q.keys(q[i, j, k].reshape(1))[0]) for j in range(N)]
            for n_, r in enumerate(orders):
                # the r-th smallest key by counting: #{key < c} <= r < #{key <= c}
                hit = [c for c in col if sum(o < c for o in col) <= r < sum(o <= c for o in col)]
                assert len(set(hit)) == 1
                assert int(Q.keys(ref[i, k, n_].reshape(1))[0]) == hit[0]
    assert np.isnan(ref[2, 0, 1])                         # +NaN is the largest
    np.testing.assert_array_equal(Q.bits(ref[:, :, 2]), Q.bits(ref[:, :, 4]))


@pytest.mark.parametrize("p", [0, 0.025, 0.16, 0.5, 0.84, 0.975, 1])
def test_interpolation_is_numpy_quantile(p):
    """The two-order interpolation against np.quantile of the float64 copy at N = 260, within
    4·2^-52·max(|lo|, |hi|)."""
    rng = np.random.default_rng(6)
    q = (rng.standard_normal((4, 260, 3)) * np.array([1, 30, 0.01]) + np.array([0, -70, 5])).astype(np.float32)
    val, bnd = Q.quantiles(q, [p])
    ref = np.quantile(q.astype(np.float64), p, axis=1).T           # (d, M)
    assert val.shape == (1, 3, 4)
    assert np.all(np.abs(val[0] - ref) <= bnd[0]), np.max(np.abs(val[0] - ref) / bnd[0])
    # and the package's rule picks the same two orders
    orders, lo_i, hi_i, frac = dfa.quantile_orders([p], 260)
    j, hi, g = Q.linear_orders(p, 260)
    assert orders[lo_i[0]] == j and orders[hi_i[0]] == hi and frac[0] == g


def test_quantile_orders():
    rng = np.random.default_rng(7)
    for N in (4, 12, 260, 1024):
        v = np.sort(rng.standard_normal(N))
        probs = [0.0, 1.0, 0.16, 0.5, 0.84, 0.025, 0.975, 1.0 / 3, 0.5]
        orders, lo_i, hi_i, frac = dfa.quantile_orders(probs, N)
        assert orders.dtype == np.int32 and np.all(np.diff(orders) > 0)            # sorted, unique
        assert orders.min() >= 0 and orders.max() <= N - 1
        assert lo_i.shape == hi_i.shape == frac.shape == (len(probs),)
        got = v[orders[lo_i]] + (v[orders[hi_i]] - v[orders[lo_i]]) * frac
        ref = np.quantile(v, probs)
        assert np.all(np.abs(got - ref) <= Q.interp_bound(v[orders[lo_i]], v[orders[hi_i]]))
        assert orders[lo_i[0]] == 0 and frac[0] == 0                                # p = 0: the minimum
        assert orders[lo_i[1]] == N - 1 == orders[hi_i[1]]                          # p = 1: the maximum itself
        assert lo_i[3] == lo_i[8] and hi_i[3] == hi_i[8]                            # a repeated probability
    # coinciding orders: N = 5, p = 0.25 and 0.5 share order 1 / 2
    orders, lo_i, hi_i, frac = dfa.quantile_orders([0.25, 0.5, 0.3], 5)
    np.testing.assert_array_equal(orders, [1, 2, 3])
    np.testing.assert_array_equal(orders[lo_i], [1, 2, 1])
    np.testing.assert_array_equal(orders[hi_i], [2, 3, 2])
    # the default probabilities at 1024 draws: six orders
    orders, _, _, _ = dfa.quantile_orders((0.16, 0.5, 0.84), 1024)
    np.testing.assert_array_equal(orders, [163, 164, 511, 512, 859, 860])
    # 33 unique orders are refused, 32 are not
    dfa.quantile_orders((np.arange(16) + 0.5) / 16, 4096)
    with pytest.raises(_lib.ArgumentError, match="at most 32"):
        dfa.quantile_orders((np.arange(17) + 0.5) / 17, 4096)
    for bad in ([1.0001], [-1e-9], [np.nan], [0.5, np.inf]):
        with pytest.raises(_lib.ArgumentError, match="probabilit"):
            dfa.quantile_orders(bad, 16)
