"""Host side of the posterior-summary call (df_pstats.hip), on CPU: df_flow_point_stats is
declared, bound and exported at ABI 5; its argument errors come back before any device work,
each with a message naming the rule; the Python wrappers refuse bad arguments before the library
is touched; the reference functions of tests/point_stats_ref.py agree with brute-force loops;
the fp64 oracle alone meets the rank bracket's cap of tests/test_gpu_point_stats.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
from densityflows_amd.data import MetaData
from helpers import spec_to_element
from train_edge_cases import SPECS, _inputs
import point_stats_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densityflows_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    m = re.search(r"^int\s+df_flow_point_stats\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "df_flow_point_stats is not declared in the header"
    assert len(m.group(1).split(",")) == 12
    res, args = _lib.SIGNATURES["df_flow_point_stats"]
    assert res is C.c_int and len(args) == 12
    assert hasattr(lib, "df_flow_point_stats"), "df_flow_point_stats is not exported"
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", src)
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION
    assert hasattr(dfa.hip.HIPChain, "run_point_stats")
    for name in ("PointStats", "posterior_stats", "sbc_ranks", "sbc_histogram"):
        assert name in flows.__all__ and hasattr(dfa, name)


def test_argument_errors_before_device_work():
    """No device exists here: every status below is returned by a check that stands before
    the first use of the handle (a non-null handle is a buffer that is never read)."""
    lib = _lib.load()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    null = C.c_void_p(0)
    out = C.c_void_p(C.addressof(C.create_string_buffer(8 * 16)))
    u = C.c_uint64

    def call(chain=fake, x=out, n_points=4, n_draws=8, chunk=0, rank=out, sums=out, draws=null):
        return lib.df_flow_point_stats(chain, x, null, n_points, n_draws, chunk, u(1), u(0), rank, sums, draws, null)

    def message():
        return lib.df_last_error().decode("utf-8")

    assert call(chain=null) == _lib.DF_ERR_INVALID and "null chain" in message()
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in message()
    assert call(chunk=-1) == _lib.DF_ERR_SHAPE and "chunk" in message()
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID, bad
        assert "multiple of 4" in message(), bad
    assert call(chunk=(1 << 24) + 1) == _lib.DF_ERR_UNSUPPORTED and "2^24" in message() and "chunk" in message()
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in message() and "n_draws" in message()
    assert call(rank=null, sums=null) == _lib.DF_ERR_INVALID and "no output" in message()
    assert call(x=null) == _lib.DF_ERR_INVALID and "rank_out needs" in message()
    # the order of df_flow_hpd_ranks: the point count before n_draws, n_draws before the outputs
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, rank=null, sums=null) == _lib.DF_ERR_INVALID and "multiple of 4" in message()
    # the same rules hold for an empty call
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, rank=null, sums=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, x=null) == _lib.DF_ERR_INVALID
    # an empty call with sound arguments runs nothing: the fake handle is never read
    assert call(n_points=0) == _lib.DF_OK
    assert call(n_points=0, x=null, rank=null) == _lib.DF_OK          # sums alone need no points
    assert call(n_points=0, x=null, rank=null, sums=null, draws=out) == _lib.DF_OK
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
    """Raised before the library is touched: Flow.hip (the only way to it) is never called."""
    flow = _flow()

    def no_device(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(dfa.Flow, "hip", no_device)
    x = np.zeros((5, 3, 2), np.float32)
    th = np.ones((1, 3, 2), np.float32)
    for fn in (lambda t, **k: dfa.posterior_stats(flow, t, x=x, seed=1, **k),
               lambda t, **k: dfa.sbc_ranks(flow, x, t, seed=1, **k)):
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
            fn((1.25,), n_draws=8)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(5, dims"):
        dfa.posterior_stats(flow, th, x=np.zeros((4, 3, 2), np.float32), seed=1)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(5, dims"):
        dfa.sbc_ranks(flow, np.zeros((4, 3, 2), np.float32), th, seed=1)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(5, dims"):
        dfa.sbc_ranks(flow, None, th, seed=1)
    # an NTuple θ has no shape of its own
    with pytest.raises(_lib.ArgumentError, match="dims="):
        dfa.posterior_stats(flow, (1.25,), seed=1)
    with pytest.raises(_lib.DimensionMismatch, match="dims"):
        dfa.posterior_stats(flow, (1.25,), x=x, dims=(2, 3), seed=1)
    with pytest.raises(AssertionError, match="the library was touched"):
        dfa.posterior_stats(flow, (1.25,), n_draws=8, dims=(3, 2), seed=1)
    with pytest.raises(AssertionError, match="the library was touched"):
        dfa.posterior_stats(flow, th, n_draws=8, seed=1)
    # an unconditional flow: θ is not looked at, the shape comes from x or dims
    flow0 = _flow("cfg2")
    with pytest.raises(_lib.ArgumentError, match="dims="):
        dfa.posterior_stats(flow0, seed=1)
    with pytest.raises(AssertionError, match="the library was touched"):
        dfa.posterior_stats(flow0, dims=(7,), n_draws=8, seed=1)


def test_sbc_histogram():
    rng = np.random.default_rng(2)
    N = 63
    r = rng.integers(0, N + 1, size=(5, 4, 11)).astype(np.int32)
    r[0, 0, :3] = [0, N, 31]
    for bins in (1, 2, 8, 64):
        h = dfa.sbc_histogram(r, N, bins)
        assert h.shape == (5, bins) and h.dtype == np.int64
        np.testing.assert_array_equal(h, P.sbc_histogram(r, N, bins))
        assert np.all(h.sum(axis=1) == 44)
    for bad in (0, -1, 3, 5, 65):
        with pytest.raises(_lib.ArgumentError, match="divide"):
            dfa.sbc_histogram(r, N, bad)
    with pytest.raises(_lib.ArgumentError, match="outside"):
        dfa.sbc_histogram(np.array([[N + 1]], np.int32), N, 8)


def test_ranks_reference():
    x = np.array([[0.0, np.nan, np.inf, -np.inf, 1.0], [1.0, 0.5, -np.inf, np.inf, np.nan]], np.float32)   # (2, 5)
    rng = np.random.default_rng(3)
    q = rng.standard_normal((5, 12, 2)).astype(np.float32)
    q[0, :4, 0] = [0.0, -0.0, np.nan, -1.0]        # ties with x = 0 count nothing, NaN counts nothing
    q[4, :3, 0] = [1.0, np.nextafter(np.float32(1), np.float32(0)), np.inf]
    r = P.ranks(x, q)
    assert r.dtype == np.int32 and r.shape == (2, 5)
    brute = np.zeros((2, 5), np.int32)
    for i in range(5):
        for k in range(2):
            for j in range(12):
                if float(q[i, j, k]) < float(x[k, i]):
                    brute[k, i] += 1
    np.testing.assert_array_equal(r, brute)
    assert r[0, 1] == 0 and r[1, 4] == 0                         # NaN coordinate
    assert r[0, 2] == 12 and r[1, 2] == 0 and r[0, 3] == 0       # ±inf coordinates
    assert r[1, 3] == 12


@pytest.mark.parametrize("d,N", [(1, 4), (5, 12), (7, 68)])
def test_sums_reference(d, N):
    rng = np.random.default_rng(d)
    M = 3
    q = (rng.standard_normal((M, N, d)) * 3 + 100).astype(np.float32)     # a mean far from 0
    block, bound = P.exact_sums(q)
    S = P.entries(d)
    assert block.shape == bound.shape == (M, S) and S == 2 * d + d * (d + 1) // 2
    for i in range(M):
        c = [float(v) for v in q[i, 0]]
        np.testing.assert_array_equal(block[i, :d], c)
        for a in range(d):
            s1 = 0.0
            for j in range(N):
                s1 += float(q[i, j, a]) - c[a]
            assert abs(s1 - block[i, d + a]) <= bound[i, d + a]
            for b in range(a + 1):
                s2 = 0.0
                for j in range(N):
                    s2 += (float(q[i, j, a]) - c[a]) * (float(q[i, j, b]) - c[b])
                e = 2 * d + a * (a + 1) // 2 + b
                assert abs(s2 - block[i, e]) <= bound[i, e], (a, b)
    assert np.all(bound[:, :d] == 0) and np.all(bound[:, d:] >= 0)
    # mean and covariance from the block: the two-pass values of the same fp64 data
    mean, cov = P.moments(block, d, N)
    pm, pc = P.plain_moments(q.astype(np.float64))
    np.testing.assert_allclose(mean, pm, rtol=1e-14, atol=0)
    np.testing.assert_allclose(cov, pc, rtol=1e-10, atol=1e-13)
    # the package's host helper is the same formula
    m2, c2 = flows.moments_from_sums(block, d, N)
    np.testing.assert_array_equal(m2, mean)
    np.testing.assert_array_equal(c2, cov)
    st = dfa.PointStats(mean, cov, None, N)
    np.testing.assert_allclose(st.std, np.sqrt(np.stack([cov[k, k] for k in range(d)])), rtol=0, atol=0)
    xt = rng.standard_normal((d, M))
    np.testing.assert_array_equal(st.zscore(xt), (mean - xt) / st.std)
    with pytest.raises(_lib.DimensionMismatch):
        st.zscore(xt[:, :2])


def test_moment_bounds_hold_for_rounded_draws():
    """The bounds of point_stats_ref.moment_bounds on a case made for them: fp64 draws, and
    their Float32 roundings standing in for a device's (within close's tolerance by far)."""
    rng = np.random.default_rng(8)
    u = rng.standard_normal((4, 68, 6)) * np.array([1, 10, 0.1, 5, 1, 2]) + np.array([0, 50, 0, -20, 3, 0])
    v = u.astype(np.float32)
    assert np.all(np.abs(v - u) <= P.H.close_tol(u))
    block, _ = P.exact_sums(v)
    mean, cov = P.moments(block, 6, 68)
    om, oc = P.plain_moments(u)
    mb, cb = P.moment_bounds(u)
    assert np.all(np.abs(mean - om) <= mb) and np.all(np.abs(cov - oc) <= cb)
    assert np.max(np.abs(cov - oc) / cb) > 1e-4          # the bound is not vacuous: within 10^4 of the error


@pytest.mark.parametrize("name", ["readme", "cfg2", "wide", "cfg5"])
def test_bracket_is_tight_for_the_oracle_alone(name):
    """The cap of tests/test_gpu_point_stats.py::test_against_oracle, Σ(hi − lo) <= 0.002 · d · M · N,
    is a property of these chains' samples and points, not of the Philox stream: the oracle
    alone meets it with numpy normal draws standing in for the device's."""
    make, d, n = SPECS[name]
    spec = make(np.random.default_rng(0))
    M, N = P.ORACLE_M, P.ORACLE_N
    x, th = _inputs(d, n, M)
    z64 = np.random.default_rng(9).standard_normal((d, M * N)).astype(np.float32).astype(np.float64)
    q64 = P.oracle_draws(spec, th, z64, N, np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32))
    lo, hi = P.rank_bracket(x, q64)
    share = np.sum(hi - lo) / (d * M * N)
    print(f"{name}: oracle bracket share {share:.6f}, lo {lo[0, :6]}, hi {hi[0, :6]}")
    assert lo.shape == hi.shape == (d, M) and np.all(lo <= hi)
    assert share <= P.UNDECIDED_CAP


def test_norm61_closed_form_reference():
    """The d = 61 chain of the GPU tests is x = A·z + b per dimension: the oracle agrees."""
    from oracle import flow_oracle as O

    spec = P.norm61_spec()
    A, b = P.norm_affine(spec)
    z = np.random.default_rng(1).standard_normal((61, 40))
    x, _ = O.forward(spec, z, np.zeros((0, 40)), np.float64)
    np.testing.assert_allclose(x, A[:, None] * z + b[:, None], rtol=1e-13, atol=1e-13)
    assert P.entries(61) == 2 * 61 + 1891
