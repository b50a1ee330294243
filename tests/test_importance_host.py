"""Host side of the importance-weight calls (df_iw.hip), on CPU: df_importance_weights and
df_draw_weighted_stats are declared, bound and exported at ABI 5; their argument errors come back
before any device work, in the stated order, each with a message naming the rule; the Python
wrappers refuse bad arguments before the library is touched; the reference functions of
tests/importance_ref.py agree with brute-force loops; weighted_moments_from_sums is
moments_from_sums at unit weights and the moments of repeated draws at integer weights."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
from densityflows_amd.data import MetaData
from helpers import spec_to_element
from train_edge_cases import SPECS
import importance_ref as I
import point_stats_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calls_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densityflows_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, n_args in (("df_importance_weights", 6), ("df_draw_weighted_stats", 9)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == n_args
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", src)
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION
    for name in ("run_importance_weights", "run_draw_weighted_stats"):
        assert name in dfa.hip.__all__ and hasattr(dfa.hip, name)
    for name in ("posterior_draws", "ImportanceWeights", "importance_weights", "WeightedPointStats",
                 "weighted_moments_from_sums", "weighted_stats", "importance_posterior_stats"):
        assert name in flows.__all__ and hasattr(dfa, name)


def _message():
    return _lib.load().df_last_error().decode("utf-8")


def _fake(n_bytes=256):
    """A non-null, 16-byte aligned pointer that is never read."""
    buf = C.create_string_buffer(n_bytes + 16)
    at = (C.addressof(buf) + 15) & ~15
    return buf, C.c_void_p(at), C.c_void_p(at + 4)


def test_importance_weights_argument_errors_before_device_work():
    """No device exists here: every status below is returned by a check that stands before the
    first launch."""
    lib = _lib.load()
    keep, ok, off = _fake()
    null = C.c_void_p(0)

    def call(logw=ok, n_points=4, n_draws=8, w=ok, stats=ok):
        return lib.df_importance_weights(logw, n_points, n_draws, w, stats, null)

    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message()
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID, bad
        assert "multiple of 4" in _message(), bad
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message() and "n_draws" in _message()
    assert call(logw=null) == _lib.DF_ERR_INVALID and "null logw" in _message()
    assert call(logw=off) == _lib.DF_ERR_INVALID and "16-byte aligned" in _message()
    assert call(w=null, stats=null) == _lib.DF_ERR_INVALID and "no output" in _message()
    assert call(n_points=1 << 61) == _lib.DF_ERR_SHAPE and "int64" in _message()
    # the order: the point count, n_draws (multiple, then size), logw, the outputs, the size
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, logw=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message()
    assert call(n_draws=(1 << 24) + 4, logw=null) == _lib.DF_ERR_UNSUPPORTED
    assert call(logw=null, w=null, stats=null) == _lib.DF_ERR_INVALID and "null logw" in _message()
    assert call(logw=off, w=null, stats=null) == _lib.DF_ERR_INVALID and "aligned" in _message()
    assert call(n_points=1 << 61, w=null, stats=null) == _lib.DF_ERR_INVALID and "no output" in _message()
    # the same rules hold for an empty call
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, logw=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, logw=off) == _lib.DF_ERR_INVALID
    assert call(n_points=0, w=null, stats=null) == _lib.DF_ERR_INVALID
    # an empty call with sound arguments launches nothing
    assert call(n_points=0) == _lib.DF_OK
    assert call(n_points=0, w=null) == _lib.DF_OK
    assert call(n_points=0, stats=null) == _lib.DF_OK
    assert call(n_points=0, w=off) == _lib.DF_OK                      # w_out has no alignment rule
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        _lib.check(call(n_draws=6))
    with pytest.raises(_lib.UnsupportedError):
        _lib.check(call(n_draws=(1 << 24) + 4))
    with pytest.raises(_lib.DimensionMismatch):
        _lib.check(call(n_points=-1))
    del keep


def test_draw_weighted_stats_argument_errors_before_device_work():
    lib = _lib.load()
    keep, ok, off = _fake()
    null = C.c_void_p(0)

    def call(xs=ok, w=ok, x=ok, d=5, n_points=4, n_draws=8, wrank=ok, sums=ok):
        return lib.df_draw_weighted_stats(xs, w, x, d, n_points, n_draws, wrank, sums, null)

    for bad in (0, -1, 65):
        assert call(d=bad) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(), bad
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message()
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID, bad
        assert "multiple of 4" in _message(), bad
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message() and "n_draws" in _message()
    assert call(xs=null) == _lib.DF_ERR_INVALID and "null xs or w" in _message()
    assert call(w=null) == _lib.DF_ERR_INVALID and "null xs or w" in _message()
    assert call(xs=off) == _lib.DF_ERR_INVALID and "16-byte aligned" in _message()
    assert call(w=off) == _lib.DF_ERR_INVALID and "16-byte aligned" in _message()
    assert call(wrank=null, sums=null) == _lib.DF_ERR_INVALID and "no output" in _message()
    assert call(x=null) == _lib.DF_ERR_INVALID and "wrank_out needs" in _message()
    assert call(n_points=1 << 58) == _lib.DF_ERR_SHAPE and "int64" in _message()
    assert call(d=64, n_points=1 << 50, n_draws=4) == _lib.DF_ERR_SHAPE           # the blocks' doubles
    # the order: d, the point count, n_draws, the inputs, the outputs, the size
    assert call(d=0, n_points=-1) == _lib.DF_ERR_INVALID and "1 .. 64" in _message()
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, xs=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message()
    assert call(xs=null, wrank=null, sums=null) == _lib.DF_ERR_INVALID and "null xs or w" in _message()
    assert call(w=off, x=null) == _lib.DF_ERR_INVALID and "aligned" in _message()
    assert call(wrank=null, sums=null, x=null) == _lib.DF_ERR_INVALID and "no output" in _message()
    assert call(n_points=1 << 58, x=null) == _lib.DF_ERR_INVALID and "wrank_out needs" in _message()
    # the same rules hold for an empty call
    assert call(n_points=0, d=65) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, xs=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, w=off) == _lib.DF_ERR_INVALID
    assert call(n_points=0, wrank=null, sums=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, x=null) == _lib.DF_ERR_INVALID
    # an empty call with sound arguments launches nothing
    assert call(n_points=0) == _lib.DF_OK
    assert call(n_points=0, x=null, wrank=null) == _lib.DF_OK         # sums alone need no points
    assert call(n_points=0, sums=null) == _lib.DF_OK
    with pytest.raises(_lib.ArgumentError, match="1 .. 64"):
        _lib.check(call(d=65))
    del keep


def _flow(name="readme"):
    make, d, n = SPECS[name]
    spec = make(np.random.default_rng(0))
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, np.full(n, -1.0, np.float32),
                                                            np.full(n, 3.0, np.float32)))


def test_python_argument_errors(monkeypatch):
    """Raised before the library is touched: the runners and Flow.hip are never called (and no
    device exists here, so a call that went on past its checks would fail in another way)."""
    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(dfa.hip, "run_importance_weights", touched)
    monkeypatch.setattr(dfa.hip, "run_draw_weighted_stats", touched)
    monkeypatch.setattr(dfa.Flow, "hip", touched)
    lt = np.zeros((3, 8), np.float32)
    # importance_weights: dtype, rank, (M, N) mismatch, N
    with pytest.raises(_lib.ArgumentError, match="log_target must be Float32"):
        dfa.importance_weights(lt.astype(np.float64))
    with pytest.raises(_lib.ArgumentError, match="log_proposal must be Float32"):
        dfa.importance_weights(lt, lt.astype(np.float64))
    for bad in (np.zeros(8, np.float32), np.zeros((3, 8, 1), np.float32)):
        with pytest.raises(_lib.DimensionMismatch, match=r"\(M, N\)"):
            dfa.importance_weights(bad)
        with pytest.raises(_lib.DimensionMismatch, match=r"\(M, N\)"):
            dfa.importance_weights(lt, bad)
    for bad in (np.zeros((3, 12), np.float32), np.zeros((2, 8), np.float32), np.zeros((8, 3), np.float32)):
        with pytest.raises(_lib.DimensionMismatch, match=r"log_proposal must have size \(3, 8\)"):
            dfa.importance_weights(lt, bad)
    for n in (6, 1023, 0):
        with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
            dfa.importance_weights(np.zeros((3, n), np.float32))
    # weighted_stats: draws, weights against draws, d, x
    q = np.zeros((3, 8, 5), np.float32)
    with pytest.raises(_lib.ArgumentError, match="draws must be Float32"):
        dfa.weighted_stats(q.astype(np.float64), lt)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(M, N, d\)"):
        dfa.weighted_stats(q[0], lt)
    with pytest.raises(_lib.ArgumentError, match="weights must be Float32"):
        dfa.weighted_stats(q, lt.astype(np.float64))
    for bad in (np.zeros((3, 12), np.float32), np.zeros((4, 8), np.float32), np.zeros(24, np.float32)):
        with pytest.raises(_lib.DimensionMismatch, match="weights"):
            dfa.weighted_stats(q, bad)
    iw = dfa.ImportanceWeights(np.ones((2, 8), np.float32), np.tile([0.0, 8.0, 8.0, 8.0], (2, 1)), 8)
    with pytest.raises(_lib.DimensionMismatch, match=r"weights must have size \(3, 8\)"):
        dfa.weighted_stats(q, iw)
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        dfa.weighted_stats(np.zeros((3, 6, 5), np.float32), np.zeros((3, 6), np.float32))
    with pytest.raises(_lib.ArgumentError, match="1 .. 64"):
        dfa.weighted_stats(np.zeros((3, 8, 65), np.float32), lt)
    for bad in (np.zeros((5, 2), np.float32), np.zeros((4, 3), np.float32), np.zeros((3, 5), np.float32)):
        with pytest.raises(_lib.DimensionMismatch, match=r"x must have size \(5, 3\)"):
            dfa.weighted_stats(q, lt, x=bad)
    with pytest.raises(_lib.DimensionMismatch, match=r"x must have size \(5, 3\)"):
        dfa.weighted_stats(q, lt, x=[[0.0, 1.0]] * 5)             # a list: converted, then checked
    # posterior_draws and importance_posterior_stats: the checks of posterior_stats
    flow = _flow()
    th = np.ones((1, 3, 2), np.float32)
    target = lambda draws, theta: touched()
    for fn in (lambda t, **k: dfa.posterior_draws(flow, t, seed=1, **k),
               lambda t, **k: dfa.importance_posterior_stats(flow, t, target, seed=1, **k)):
        for bad in ((1.0, 2.0), (), None, np.ones((2, 3, 2), np.float32)):
            with pytest.raises(AssertionError, match="dimensions θ"):
                fn(bad)
        for bad in (0, -4, 6, 1023):
            with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
                fn(th, n_draws=bad)
        with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
            fn(th, n_draws=(1 << 24) + 4)
        with pytest.raises(_lib.ArgumentError, match="dims="):
            fn((1.25,))
        with pytest.raises(AssertionError, match="dimensions θ"):
            fn(th, dims=(2, 3))
        with pytest.raises(AssertionError, match="the library was touched"):
            fn(th, n_draws=8)
        with pytest.raises(AssertionError, match="the library was touched"):
            fn((1.25,), n_draws=8, dims=(3, 2))
    with pytest.raises(_lib.DimensionMismatch, match=r"\(5, dims"):
        dfa.importance_posterior_stats(flow, th, target, x=np.zeros((4, 3, 2), np.float32), seed=1)
    with pytest.raises(AssertionError, match="dimensions θ"):
        dfa.importance_posterior_stats(flow, th, target, x=np.zeros((5, 2, 3), np.float32), seed=1)


def _logw_cases():
    rng = np.random.default_rng(4)
    lw = rng.uniform(-30, 0, (6, 12)).astype(np.float32)
    lw[1, 2:5] = -np.inf                          # weight 0
    lw[2, 7] = np.nan                             # NaN in its point only
    lw[3, :] = -np.inf                            # a point without weight
    lw[4, 3] = np.inf
    lw[5, :] = np.float32(-3.25)                  # constant: unit weights
    return lw


def test_weights_reference():
    lw = _logw_cases()
    m, w = I.weights64(lw)
    M, N = lw.shape
    for i in range(M):
        best = None
        for v in lw[i]:
            if not math.isnan(float(v)) and (best is None or float(v) > best):
                best = float(v)
        assert float(m[i]) == best
        for j in range(N):
            diff = np.float32(lw[i, j]) - np.float32(m[i]) if not (np.isinf(lw[i, j]) and np.isinf(m[i])) else np.nan
            ref = math.exp(float(diff)) if not math.isnan(float(diff)) else math.nan
            # (two fp64 exp routines, each within an ulp of the value)
            assert (math.isnan(ref) and math.isnan(w[i, j])) or abs(ref - w[i, j]) <= 2.0 ** -51 * ref, (i, j)
    assert np.all(w[1, 2:5] == 0) and np.all(np.isfinite(w[[0, 1, 5]]))
    assert np.isnan(w[2, 7]) and np.sum(np.isnan(w[2])) == 1
    assert np.all(np.isnan(w[3])) and m[3] == -np.inf
    assert m[4] == np.inf and np.isnan(w[4, 3]) and np.all(np.delete(w[4], 3) == 0)
    assert np.all(w[5] == 1.0) and m[5] == np.float32(-3.25)
    # the sums of the Float32 weights, exact, against a plain loop
    w32 = w.astype(np.float32)
    stats, bound = I.weight_sums(w32)
    for i in range(M):
        s1 = s2 = 0.0
        pos = 0
        for v in w32[i]:
            s1 += float(v)
            s2 += float(v) * float(v)
            pos += 1 if v > 0 else 0
        assert stats[i, 2] == pos
        if np.all(np.isfinite(w32[i])):
            assert abs(s1 - stats[i, 0]) <= bound[i, 0] and abs(s2 - stats[i, 1]) <= bound[i, 1]
        else:
            assert np.isnan(stats[i, 0]) and np.isnan(stats[i, 1])
    assert stats[1, 2] == N - 3 and stats[2, 2] == N - 1 and stats[3, 2] == 0 and stats[4, 2] == 0
    assert list(stats[5]) == [N, N, N]
    # evidence, standard error and ESS; the class forms the same numbers
    lz, se, ess = I.evidence(m, stats[:, 0], stats[:, 1], N)
    assert lz[5] == float(np.float32(-3.25)) and ess[5] == N and se[5] == 0.0
    i = 0
    assert lz[i] == float(m[i]) + math.log(stats[i, 0] / N)
    assert ess[i] == stats[i, 0] ** 2 / stats[i, 1] and 1.0 <= ess[i] <= N
    assert se[i] == math.sqrt((N * stats[i, 1] / stats[i, 0] ** 2 - 1.0) / (N - 1))
    iw = dfa.ImportanceWeights(w32, np.column_stack([m.astype(np.float64), stats]), N)
    for got, ref in ((iw.log_evidence, lz), (iw.log_evidence_stderr, se), (iw.ess, ess), (iw.efficiency, ess / N)):
        np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(iw.n_positive, stats[:, 2].astype(np.int64))
    assert iw.n_positive.dtype == np.int64
    nz = iw.normalized()
    assert nz.dtype == np.float64 and nz.shape == (M, N)
    np.testing.assert_allclose(nz[[0, 1, 5]].sum(axis=1), 1.0, rtol=1e-14)


def test_weighted_ranks_reference():
    x = np.array([[0.0, np.nan, np.inf, -np.inf, 1.0], [1.0, 0.5, -np.inf, np.inf, np.nan]], np.float32)   # (2, 5)
    rng = np.random.default_rng(3)
    q = rng.standard_normal((5, 12, 2)).astype(np.float32)
    q[0, :4, 0] = [0.0, -0.0, np.nan, -1.0]        # ties with x = 0 count nothing, NaN counts nothing
    q[4, :3, 0] = [1.0, np.nextafter(np.float32(1), np.float32(0)), np.inf]
    w = rng.uniform(0, 1, (5, 12)).astype(np.float32)
    w[2, 5] = 0.0
    r, bound = I.weighted_ranks(x, q, w)
    assert r.shape == bound.shape == (2, 5)
    for i in range(5):
        for k in range(2):
            s = 0.0
            for j in range(12):
                if float(q[i, j, k]) < float(x[k, i]):
                    s += float(w[i, j])
            assert abs(s - r[k, i]) <= bound[k, i]
    assert r[0, 1] == 0 and r[1, 4] == 0                         # NaN coordinate
    assert r[1, 2] == 0 and r[0, 3] == 0                         # −inf coordinates
    assert abs(r[0, 2] - math.fsum(float(v) for v in w[2])) <= bound[0, 2]      # +inf: every weight
    # unit weights: the integer ranks
    np.testing.assert_array_equal(I.weighted_ranks(x, q, np.ones((5, 12), np.float32))[0], P.ranks(x, q))


@pytest.mark.parametrize("d,N", [(1, 4), (5, 12), (7, 68)])
def test_weighted_sums_reference(d, N):
    rng = np.random.default_rng(d)
    M = 3
    q = (rng.standard_normal((M, N, d)) * 3 + 100).astype(np.float32)     # a mean far from 0
    w = rng.uniform(0, 1, (M, N)).astype(np.float32)
    w[0, 1] = 0.0
    block, bound = I.weighted_exact_sums(q, w)
    S = I.block_entries(d)
    assert block.shape == bound.shape == (M, S) and S == 2 + 2 * d + d * (d + 1) // 2
    for i in range(M):
        c = [float(v) for v in q[i, 0]]
        np.testing.assert_array_equal(block[i, 2:2 + d], c)
        w1 = w2 = 0.0
        for j in range(N):
            w1 += float(w[i, j])
            w2 += float(w[i, j]) ** 2
        assert abs(w1 - block[i, 0]) <= bound[i, 0] and abs(w2 - block[i, 1]) <= bound[i, 1]
        for a in range(d):
            s1 = 0.0
            for j in range(N):
                s1 += float(w[i, j]) * (float(q[i, j, a]) - c[a])
            assert abs(s1 - block[i, 2 + d + a]) <= bound[i, 2 + d + a]
            for b in range(a + 1):
                s2 = 0.0
                for j in range(N):
                    s2 += float(w[i, j]) * (float(q[i, j, a]) - c[a]) * (float(q[i, j, b]) - c[b])
                e = 2 + 2 * d + a * (a + 1) // 2 + b
                assert abs(s2 - block[i, e]) <= bound[i, e], (a, b)
    assert np.all(bound[:, 2:2 + d] == 0) and np.all(bound >= 0)
    # unit weights: the block of point_stats_ref behind W1 = W2 = N
    ub, _ = I.weighted_exact_sums(q, np.ones((M, N), np.float32))
    np.testing.assert_array_equal(ub[:, 2:], P.exact_sums(q)[0])
    assert np.all(ub[:, :2] == N)
    # mean and covariance from the block: the package's helper is the textbook form
    mean, cov = I.weighted_moments(block, d)
    m2, c2, ess = flows.weighted_moments_from_sums(block, d)
    np.testing.assert_allclose(m2, mean, rtol=1e-14, atol=0)
    np.testing.assert_allclose(c2, cov, rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(ess, block[:, 0] ** 2 / block[:, 1])
    wn = w.astype(np.float64) / w.astype(np.float64).sum(axis=1, keepdims=True)
    q64 = q.astype(np.float64)
    pm = np.einsum("mj,mjk->km", wn, q64)
    np.testing.assert_allclose(mean, pm, rtol=1e-13, atol=0)
    r = q64 - pm.T[:, None, :]
    pc = np.einsum("mj,mja,mjb->abm", wn, r, r) / (1.0 - np.sum(wn * wn, axis=1))
    np.testing.assert_allclose(cov, pc, rtol=1e-9, atol=1e-12)
    st = dfa.WeightedPointStats(m2, c2, None, ess, N)
    np.testing.assert_array_equal(st.std, np.sqrt(np.stack([c2[k, k] for k in range(d)])))
    xt = rng.standard_normal((d, M))
    np.testing.assert_array_equal(st.zscore(xt), (m2 - xt) / st.std)
    with pytest.raises(_lib.DimensionMismatch):
        st.zscore(xt[:, :2])


@pytest.mark.parametrize("d,N", [(1, 4), (5, 12), (7, 68)])
def test_weighted_moments_from_sums(d, N):
    rng = np.random.default_rng(10 + d)
    M = 4
    q = (rng.standard_normal((M, N, d)) * 3 + 100).astype(np.float32)
    # unit weights: moments_from_sums bit for bit at ddof = 1
    ub, _ = I.weighted_exact_sums(q, np.ones((M, N), np.float32))
    pb, _ = P.exact_sums(q)
    mean, cov, ess = flows.weighted_moments_from_sums(ub, d, ddof=1)
    pm, pc = flows.moments_from_sums(pb, d, N)
    np.testing.assert_array_equal(mean.view(np.uint64), pm.view(np.uint64))
    np.testing.assert_array_equal(np.ascontiguousarray(cov).view(np.uint64), np.ascontiguousarray(pc).view(np.uint64))
    assert np.all(ess == N)
    # integer weights are frequencies: the plain moments of the draws repeated that many times —
    # the mean at either ddof, the covariance at ddof = 0 (the reliability correction 1 − W2/W1² of
    # ddof = 1 is not the frequency correction 1 − 1/Σn, so the two differ there by construction)
    counts = rng.integers(0, 5, (M, N))
    counts[:, 0] = 1
    ib, _ = I.weighted_exact_sums(q, counts.astype(np.float32))
    rm, rc = I.repeated_moments(q, counts, ddof=0)
    m0, c0, _ = flows.weighted_moments_from_sums(ib, d, ddof=0)
    m1, c1, e1 = flows.weighted_moments_from_sums(ib, d, ddof=1)
    np.testing.assert_allclose(m0, rm, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(m1, m0)
    np.testing.assert_allclose(c0, rc, rtol=1e-12, atol=0)
    tot = counts.sum(axis=1).astype(np.float64)
    corr = 1.0 - (counts ** 2).sum(axis=1) / tot ** 2
    np.testing.assert_allclose(c1, c0 / corr, rtol=1e-13, atol=0)
    np.testing.assert_allclose(e1, tot ** 2 / (counts ** 2).sum(axis=1), rtol=1e-15)
