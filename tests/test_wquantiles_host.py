"""Host side of the weighted quantile and histogram calls (df_wquant.hip, df_whist.hip), on CPU:
the three calls are declared, bound and exported; their argument errors come back before any
device work, in the documented order; the Python wrappers refuse bad probabilities, shapes and
tables before the library is touched; the pure-integer references of tests/wquantile_ref.py agree
with each other, with the unweighted references at unit weights and with numpy's weighted
inverted-CDF quantile; and the host planner at a bin width of two words (df_hist_plan.cpp,
printed by tests/whist_plan_check.cpp) keeps its invariants."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
import histogram_ref as H
import quantile_ref as Q
import resample_ref as R
import test_plan_fingerprint as PF
import wquantile_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 32


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densityflows_hip.h")).read(), flags=re.S)


def test_calls_declared_bound_and_exported():
    src = _header()
    lib = _lib.load()
    for name, count in (("df_draw_weight_scale", 5), ("df_draw_weighted_quantiles", 10),
                        ("df_draw_weighted_histograms", 12)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == count
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == count
        assert hasattr(lib, name), f"{name} is not exported"
    for macro, value in (("DF_WQUANT_MAX_PROBS", dfa.WQUANT_MAX_PROBS), ("DF_WHIST_MAX_TABLE_BINS", dfa.WHIST_MAX_TABLE_BINS)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", src)
        assert m and int(m.group(1)) == value, macro
    assert dfa.WQUANT_MAX_PROBS == 32 and dfa.WHIST_MAX_TABLE_BINS == 8192
    for name in ("run_draw_weight_scale", "run_draw_weighted_quantiles", "run_draw_weighted_histograms"):
        assert hasattr(dfa.hip, name)
    for name in ("quantile_numerators", "weight_scale", "weighted_quantiles", "weighted_credible_intervals",
                 "weighted_histograms", "WeightedPointHistograms", "importance_posterior_quantiles",
                 "importance_credible_intervals", "importance_posterior_histograms"):
        assert name in flows.__all__ and hasattr(dfa, name)


def _i32(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def _u64(*v):
    return (C.c_uint64 * max(len(v), 1))(*v)


def _message(lib):
    return lib.df_last_error().decode("utf-8")


def _pointers():
    buf = C.create_string_buffer(1024)
    base = (C.addressof(buf) + 15) & ~15
    return buf, base, [C.c_void_p(base + 64 * k) for k in range(6)], C.c_void_p(0)


def test_weight_scale_argument_errors_before_device_work():
    lib = _lib.load()
    buf, base, (w, out, *_), null = _pointers()

    def call(w=w, n_points=4, n_draws=8, out=out):
        return lib.df_draw_weight_scale(w, n_points, n_draws, out, null)

    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message(lib)
    for bad in (0, -4, 6):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib)
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib)
    assert call(w=null) == _lib.DF_ERR_INVALID and "null" in _message(lib)
    assert call(out=null) == _lib.DF_ERR_INVALID and "null" in _message(lib)
    assert call(w=C.c_void_p(base + 4)) == _lib.DF_ERR_INVALID and "16-byte" in _message(lib)
    assert call(n_points=1 << 60) == _lib.DF_ERR_SHAPE and "int64" in _message(lib)
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, w=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib)
    assert call(n_points=0, w=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0) == _lib.DF_OK


def test_weighted_quantiles_argument_errors_before_device_work():
    """No device exists here: every status below is returned before anything is launched."""
    lib = _lib.load()
    buf, base, (xs, w, out, sc, *_), null = _pointers()

    def call(xs=xs, w=w, d=3, n_points=4, n_draws=8, nums=_u64(0, ONE // 2, ONE), n_probs=3, out=out, sc=sc):
        return lib.df_draw_weighted_quantiles(xs, w, d, n_points, n_draws, nums, n_probs, out, sc, null)

    for bad in (0, -1, 65):
        assert call(d=bad) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(lib), bad
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message(lib)
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib), bad
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib)
    for name in ("xs", "w", "out", "sc"):
        assert call(**{name: null}) == _lib.DF_ERR_INVALID and "null" in _message(lib), name
    assert call(nums=None) == _lib.DF_ERR_INVALID and "null nums" in _message(lib)
    for off in (4, 8, 12):
        assert call(xs=C.c_void_p(base + off)) == _lib.DF_ERR_INVALID and "xs must be 16-byte" in _message(lib)
        assert call(w=C.c_void_p(base + 64 + off)) == _lib.DF_ERR_INVALID and "w must be 16-byte" in _message(lib)
    for bad in (0, -1, 33):
        assert call(n_probs=bad) == _lib.DF_ERR_UNSUPPORTED and "n_probs" in _message(lib), bad
    assert call(nums=_u64(0, ONE + 1, ONE)) == _lib.DF_ERR_INVALID and "nums[1]" in _message(lib)
    assert call(nums=_u64(0, 1, (1 << 64) - 1)) == _lib.DF_ERR_INVALID and "nums[2]" in _message(lib)
    assert call(n_points=1 << 60) == _lib.DF_ERR_SHAPE and "int64" in _message(lib)
    # the order of the checks: each rule before the next
    assert call(d=0, n_points=-1) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(lib)
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, xs=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib)
    assert call(xs=null, w=C.c_void_p(base + 68)) == _lib.DF_ERR_INVALID and "null" in _message(lib)
    assert call(w=C.c_void_p(base + 68), n_probs=0) == _lib.DF_ERR_INVALID and "16-byte" in _message(lib)
    assert call(n_probs=33, nums=_u64(ONE + 1)) == _lib.DF_ERR_UNSUPPORTED
    assert call(nums=_u64(0, ONE + 1, ONE), n_points=1 << 60) == _lib.DF_ERR_INVALID and "nums[1]" in _message(lib)
    # the same rules hold for an empty call, which then launches nothing
    assert call(n_points=0, d=0) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, xs=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_probs=33) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, nums=_u64(0, ONE + 1, ONE)) == _lib.DF_ERR_INVALID
    assert call(n_points=0) == _lib.DF_OK
    assert call(n_points=0, n_probs=32, nums=_u64(*range(32))) == _lib.DF_OK


CORNER3 = _i32(0, -1, 1, -1, 2, -1, 0, 1, 0, 2, 1, 2)        # d = 3: 6 tables


def test_weighted_histograms_argument_errors_before_device_work():
    lib = _lib.load()
    buf, base, (xs, w, ed, out, sc, _), null = _pointers()

    def call(xs=xs, w=w, d=3, n_points=4, n_draws=8, edges=ed, bins=_i32(4, 5, 6), keep=CORNER3, n_tables=6, out=out,
             sc=sc):
        return lib.df_draw_weighted_histograms(xs, w, d, n_points, n_draws, edges, bins, keep, n_tables, out, sc, null)

    for bad in (0, -1, 65):
        assert call(d=bad) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(lib), bad
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message(lib)
    for bad in (0, -4, 6):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib), bad
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib)
    for name in ("xs", "w", "out", "sc", "edges"):
        assert call(**{name: null}) == _lib.DF_ERR_INVALID and "null" in _message(lib), name
    assert call(bins=None) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    assert call(keep=None) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    assert call(xs=C.c_void_p(base + 4)) == _lib.DF_ERR_INVALID and "xs must be 16-byte" in _message(lib)
    assert call(w=C.c_void_p(base + 72)) == _lib.DF_ERR_INVALID and "w must be 16-byte" in _message(lib)
    for bad in (0, -1, 2081):
        assert call(n_tables=bad) == _lib.DF_ERR_UNSUPPORTED and "n_tables" in _message(lib), bad
    assert call(bins=_i32(4, -1, 6)) == _lib.DF_ERR_INVALID and "bins[1]" in _message(lib)
    assert call(bins=_i32(4, 5, 129)) == _lib.DF_ERR_UNSUPPORTED and "bins[2]" in _message(lib)
    one = lambda a, b: dict(keep=_i32(0, -1, a, b), n_tables=2)
    assert call(**one(3, -1)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib) and "first" in _message(lib)
    assert call(**one(2, 1)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib)
    assert call(**one(0, -1)) == _lib.DF_ERR_INVALID and "repeats" in _message(lib)
    assert call(bins=_i32(4, 0, 6), **one(1, 2)) == _lib.DF_ERR_INVALID and "without bins" in _message(lib)
    # the new rule: a table above 8192 bins, named by its request
    big = dict(d=2, bins=_i32(91, 91), keep=_i32(0, -1, 0, 1), n_tables=2)
    assert call(**big) == _lib.DF_ERR_UNSUPPORTED
    assert "keep[1] = {0, 1}" in _message(lib) and "8281" in _message(lib) and "8192" in _message(lib)
    assert call(d=2, bins=_i32(128, 128), keep=_i32(0, 1), n_tables=1) == _lib.DF_ERR_UNSUPPORTED
    # sizes: T = 89 words of 8 bytes
    assert call(n_points=(1 << 61) // 89) == _lib.DF_ERR_SHAPE and "int64" in _message(lib)
    # the order of the checks
    assert call(d=0, n_points=-1) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(lib)
    assert call(n_draws=6, xs=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib)
    assert call(xs=null, n_tables=0) == _lib.DF_ERR_INVALID and "null" in _message(lib)
    assert call(w=C.c_void_p(base + 72), n_tables=0) == _lib.DF_ERR_INVALID and "16-byte" in _message(lib)
    assert call(n_tables=0, bins=_i32(4, -1, 6)) == _lib.DF_ERR_UNSUPPORTED and "n_tables" in _message(lib)
    assert call(d=2, bins=_i32(91, 91), keep=_i32(0, 1, 0, 1), n_tables=2) == _lib.DF_ERR_INVALID and "repeats" in _message(lib)
    assert call(n_points=(1 << 61) // 8281, **big) == _lib.DF_ERR_UNSUPPORTED and "8192" in _message(lib)
    # an empty call: the same rules, then DF_OK with nothing launched
    assert call(n_points=0, d=0) == _lib.DF_ERR_INVALID
    assert call(n_points=0, w=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_tables=0) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, **big) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0) == _lib.DF_OK
    assert call(n_points=0, d=2, bins=_i32(90, 90), keep=_i32(0, 1), n_tables=1) == _lib.DF_OK
    k64 = [v for K in H.corner([4] * 64) for v in (K + (-1,))[:2]]
    assert call(n_points=0, d=64, bins=_i32(*([4] * 64)), keep=_i32(*k64), n_tables=2080) == _lib.DF_OK


def test_python_wrappers_refuse_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("library touched")))
    assert dfa.quantile_numerators((0.0, 0.5, 1.0, 0.16)) == [0, 1 << 31, ONE, int(np.rint(np.float64(0.16) * 2.0 ** 32))]
    assert dfa.quantile_numerators(0.25) == [1 << 30]
    for bad in ((-0.1,), (1.0000001,), (np.nan,), (0.5, np.inf), (), np.linspace(0, 1, 33)):
        with pytest.raises(_lib.ArgumentError):
            dfa.quantile_numerators(bad)
    assert len(dfa.quantile_numerators(np.linspace(0, 1, 32))) == 32
    x = np.zeros((2, 8, 3), np.float32)
    w = np.ones((2, 8), np.float32)
    with pytest.raises(_lib.ArgumentError, match="Float32"):
        dfa.weighted_quantiles(x.astype(np.float64), w)
    with pytest.raises(_lib.ArgumentError, match="Float32"):
        dfa.weighted_quantiles(x, w.astype(np.float64))
    with pytest.raises(_lib.DimensionMismatch):
        dfa.weighted_quantiles(x[0], w)
    with pytest.raises(_lib.DimensionMismatch):
        dfa.weighted_quantiles(x, w[:, :4])
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        dfa.weighted_quantiles(x[:, :6], w[:, :6])
    with pytest.raises(_lib.ArgumentError, match="1 .. 64"):
        dfa.weighted_quantiles(np.zeros((2, 8, 65), np.float32), w)
    with pytest.raises(_lib.ArgumentError, match=r"\[0, 1\]"):
        dfa.weighted_quantiles(x, w, probs=(0.5, 1.5))
    with pytest.raises(_lib.ArgumentError, match="level"):
        dfa.weighted_credible_intervals(x, w, level=1.0)
    with pytest.raises(_lib.DimensionMismatch):
        dfa.weight_scale(np.ones(8, np.float32))
    with pytest.raises(_lib.ArgumentError, match="Float32"):
        dfa.weight_scale(np.ones((2, 8)))
    edges = [(-1.0, 1.0, 4), None, (-1.0, 1.0, 4)]
    with pytest.raises(_lib.DimensionMismatch):
        dfa.weighted_histograms(x, w[:1], edges)
    with pytest.raises(_lib.ArgumentError, match="without edges"):
        dfa.weighted_histograms(x, w, edges, keep=[(1,)])
    with pytest.raises(_lib.UnsupportedError, match="8192"):
        dfa.weighted_histograms(x, w, [(-1.0, 1.0, 91), (-1.0, 1.0, 91), None])


def test_weighted_point_histograms_arithmetic():
    edges = [np.array([0.0, 1.0, 3.0], np.float32), None]
    tabs = {(0,): np.array([[1 << 31, 3 << 31], [0, 0], [5, 7]], np.uint64)}
    ph = flows.WeightedPointHistograms(tabs, edges, [1, 0, -3], [4 << 31, 0, 16], 8)
    assert ph.sums(0).dtype == np.uint64 and ph.sums((0,)) is tabs[(0,)]
    np.testing.assert_array_equal(ph.mass(0), [[1.0, 3.0], [0.0, 0.0], [5 * 2.0 ** -35, 7 * 2.0 ** -35]])
    np.testing.assert_array_equal(ph.inside(0), np.array([4 << 31, 0, 12], np.uint64))
    den = ph.density(0)
    np.testing.assert_array_equal(den[0], [0.25, 0.375])
    assert np.isnan(den[1]).all()
    np.testing.assert_array_equal(den[2], [5 / 16, 7 / 32])
    np.testing.assert_array_equal(ph.pooled(0), [0.25 + 5 / 16, 0.75 + 7 / 16])
    assert "tables=1" in repr(ph)


# ---------------------------------------------------------------------------
# the integer references
# ---------------------------------------------------------------------------

def _cases():
    rng = np.random.default_rng(20260)
    for N in (4, 12, 64, 68, 260):
        M, d = 5, 3
        x = W.plant_draws(rng.standard_normal((M, N, d)).astype(np.float32), rng)
        for name, w in W.weight_patterns(M, N, rng).items():
            yield f"{name} N={N}", x, w


CASES = list(_cases())
NUMS = [0, 1, ONE // 7, ONE // 2, ONE - 1, ONE, W.numerators([0.16])[0], W.numerators([0.84])[0]]


def test_scale_matches_frexp_and_the_quantiser():
    for name, x, w in CASES:
        e, T, q = W.scales(w)
        for i in range(w.shape[0]):
            assert q[i].tolist() == R.quantise(w[i])
            if T[i] == 0:
                assert e[i] == 0 and not q[i].any(), name
                continue
            with np.errstate(invalid="ignore"):
                part = np.isfinite(w[i]) & (w[i] > 0)
            wmax = float(w[i][part].max())
            assert 0.5 <= wmax * 2.0 ** -float(e[i]) < 1.0
            assert (1 << 31) <= int(q[i].max()) <= ONE and 0 < T[i] < 1 << 56
            assert not q[i][~part].any()
    assert "hostile N=64" in [c[0] for c in CASES]
    e, T, _ = W.scales(np.array([[1e-45, 0, 0, 0], [3.4028235e38, 1, 1, 1], [1, 1, 1, 1]], np.float32))
    assert e.tolist() == [-148, 128, 1] and T.tolist() == [1 << 31, (1 << 32) - 256, 1 << 33]


def test_scan_radix_and_vector_references_agree():
    for name, x, w in CASES:
        M, N, d = x.shape
        vec = W.quantiles(x, w, NUMS).view(np.uint32)
        for i in range(M):
            _, T, q = W.scale(w[i])
            for k in range(d):
                for p, num in enumerate(NUMS):
                    a = W.quantile_scan(x[i, :, k], q, num)
                    assert a == W.quantile_radix(x[i, :, k], q, num) == int(vec[i, k, p]), (name, i, k, num)
                    if T == 0:
                        assert a == W.NAN_BITS
                    else:                                       # a draw with q > 0, or one that shares its bits
                        hit = x[i, :, k].view(np.uint32) == a
                        assert hit.any() and any(q[j] > 0 for j in np.flatnonzero(hit)), (name, i, k, num)


def test_ends_and_one_weight_that_carries_everything():
    rng = np.random.default_rng(3)
    x = W.plant_draws(rng.standard_normal((4, 64, 2)).astype(np.float32), rng)
    w = W.weight_patterns(4, 64, rng)
    for name in ("lognormal3", "hostile", "lognormal30"):
        _, T, q = W.scales(w[name])
        out = W.quantiles(x, w[name], [0, ONE]).view(np.uint32)
        for i in range(4):
            if T[i] == 0:
                assert (out[i] == W.NAN_BITS).all()
                continue
            part = q[i] > 0
            for k in range(2):
                keys = Q.keys(x[i, part, k])
                assert out[i, k, 0] == Q.values(keys.min()[None]).view(np.uint32)[0]
                assert out[i, k, 1] == Q.values(keys.max()[None]).view(np.uint32)[0]
    hot = w["onehot"]
    out = W.quantiles(x, hot, NUMS).view(np.uint32)
    at = np.argmax(hot, axis=1)
    for i in range(4):
        assert (out[i] == x[i, at[i]].view(np.uint32)[:, None]).all()


@pytest.mark.parametrize("N", [4, 64, 256, 1024])
def test_unit_weight_identities(N):
    rng = np.random.default_rng(N)
    M, d = 3, 4
    x = W.plant_draws(rng.standard_normal((M, N, d)).astype(np.float32), rng)
    w = np.ones((M, N), np.float32)
    e, T, q = W.scales(w)
    assert (e == 1).all() and (q == 1 << 31).all() and (T == N << 31).all()
    orders = sorted({0, 1, N // 2, N - 1})
    nums = [(r + 1) * ONE // N for r in orders]
    np.testing.assert_array_equal(W.quantiles(x, w, nums).view(np.uint32), Q.order_stats(x, orders).view(np.uint32))
    edges = [np.linspace(-2, 2, 9).astype(np.float32), None, np.array([-np.inf, 0, np.inf], np.float32),
             np.linspace(-1, 1, 4).astype(np.float32)]
    keep = H.corner(H.bins_of(edges))
    np.testing.assert_array_equal(W.blocks(x, w, edges, keep), H.blocks(x, edges, keep).astype(np.uint64) << np.uint64(31))


def test_weighted_blocks_against_the_brute_loop_and_mass_conservation():
    rng = np.random.default_rng(8)
    M, N, d = 4, 24, 3
    edges = [np.array([-1.5, -0.5, 0.0, 0.75, 2.0], np.float32), np.array([-np.inf, np.inf], np.float32),
             np.linspace(-1, 1, 4).astype(np.float32)]
    x = H.plant(rng.standard_normal((M, N, d)).astype(np.float32), edges, rng)
    keep = H.corner(H.bins_of(edges))
    for name, w in W.weight_patterns(M, N, rng).items():
        a = W.blocks(x, w, edges, keep)
        np.testing.assert_array_equal(a, W.blocks_brute(x, w, edges, keep), err_msg=name)
        _, T, q = W.scales(w)
        nan_q = (q * np.isnan(x[:, :, 1])).sum(axis=1, dtype=np.uint64)
        np.testing.assert_array_equal(a[:, 4], T.astype(np.uint64) - nan_q)       # the (−inf, +inf) table of dimension 1
        assert (a.sum(axis=1)[T == 0] == 0).all()


def test_against_numpy_inverted_cdf():
    """np.quantile(weights=q, method="inverted_cdf") on the quantised weights, at probabilities whose
    num·T/2^32 lies at least 1 away from every cumulative sum (numpy forms p·T in float64)."""
    rng = np.random.default_rng(11)
    checked = 0
    for N in (4, 12, 64, 260):
        x = rng.standard_normal((3, N, 2)).astype(np.float32)
        x[:, : N // 4, :] = np.float32(0.25)                    # tied draws
        w = np.exp(rng.standard_normal((3, N))).astype(np.float32)
        w[:, 1] = 0.0
        w[:, 2] = np.nan
        _, T, q = W.scales(w)
        for i in range(3):
            for k in range(2):
                order = np.argsort(Q.keys(x[i, :, k]), kind="stable")
                cum = [int(v) for v in np.cumsum(q[i][order], dtype=np.uint64)]
                for p in rng.uniform(0, 1, 16):
                    num = W.numerators([p])[0]
                    target = num * int(T[i]) / ONE
                    if min(abs(target - c) for c in cum + [0]) < 1.0:
                        continue
                    want = np.quantile(x[i, :, k].astype(np.float64), num / ONE, weights=q[i].astype(np.float64),
                                       method="inverted_cdf")
                    got = W.quantiles(x[i:i + 1, :, k:k + 1], w[i:i + 1], [num])[0, 0, 0]
                    assert np.float64(got) == want, (N, i, k, p)
                    checked += 1
    assert checked > 300


# ---------------------------------------------------------------------------
# the host planner at two words per bin
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("whist_plan"))
    exe = PF.compile_program(os.path.join(PF.CSRC, "df_hist_plan.cpp"), os.path.join(work, "whist_plan_check"),
                             program="whist_plan_check.cpp")
    count = [0]

    def run(d, bins, keep, teams, n_points=1):
        count[0] += 1
        path = os.path.join(work, f"case{count[0]}.txt")
        with open(path, "w") as f:
            f.write(f"{d} {teams} {len(keep)} {n_points}\n" + " ".join(str(int(b)) for b in bins) + "\n" +
                    "\n".join(f"{K[0]} {K[1] if len(K) == 2 else -1}" for K in keep) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout.splitlines()

    return run


def _parse(lines):
    head = {ln.split()[0]: ln.split()[1:] for ln in lines if ln.split()[0] in ("check", "plan", "budget", "message")}
    groups = []
    for ln in lines:
        w = ln.split()
        if w[0] == "group":
            groups.append({"head": [int(v) for v in w[1:]], "dims": [], "tables": []})
        elif w[0] == "dim":
            groups[-1]["dims"].append(tuple(int(v) for v in w[1:]))
        elif w[0] == "table":
            groups[-1]["tables"].append(tuple(int(v) for v in w[1:]))
    return head, groups


def _check_plan(lines, d, bins, keep, teams):
    """Every requested table in exactly one group; every group within the budgets at two words per
    bin; the offsets tile [0, T) in request order; a group's tables tile its LDS part in bins."""
    head, groups = _parse(lines)
    assert int(head["check"][0]) == 0, head
    T = sum(H.sizes(keep, bins))
    assert int(head["check"][1]) == T and int(head["plan"][2]) == T
    assert int(head["plan"][0]) == 1 and int(head["plan"][1]) == len(groups) >= 1
    lds_words, table_words, max_dims, max_tables = (int(v) for v in head["budget"])
    assert lds_words * 4 * 2 <= 160 * 1024 and table_words * 4 == 64 * 1024
    want_off = dict(zip([(K[0], K[1] if len(K) == 2 else -1) for K in keep], np.concatenate([[0], np.cumsum(H.sizes(keep, bins))])))
    seen = {}
    for g in groups:
        n_dims, n_tables, edge_words, tw, lds = g["head"]
        assert 1 <= n_dims == len(g["dims"]) <= max_dims and 1 <= n_tables == len(g["tables"]) <= max_tables
        assert lds <= lds_words and teams * tw <= table_words and tw % 4 == 0
        assert lds == 64 + (edge_words + 3) // 4 * 4 + teams * tw + 4 * 64 * (n_dims | 1)
        mine = {dim for dim, *_ in g["dims"]}
        assert sum(L + 1 for _, L, _, _ in g["dims"]) == edge_words
        at = 0
        for a, b, out_off, lds_off in g["tables"]:
            assert a in mine and (b == -1 or (b in mine and a < b))
            assert (a, b) not in seen, "a table in two groups"
            seen[(a, b)] = out_off
            assert out_off == want_off[(a, b)] and lds_off == at
            at += bins[a] * (bins[b] if b >= 0 else 1)
        assert 2 * at <= tw < 2 * at + 4
    assert set(seen) == set(want_off), "a requested table in no group"
    return groups


WPLAN_CASES = {
    "d = 5 corner at 32 bins": (5, [32] * 5, None),
    "d = 32 corner at 32 bins": (32, [32] * 32, None),
    "d = 64 corner at 32 bins": (64, [32] * 64, None),
    "d = 64 corner at 4 bins": (64, [4] * 64, None),
    "d = 61 corner at 8 bins": (61, [8] * 61, None),
    "one 90 x 90 table": (3, [90, 0, 90], [(0, 2)]),
    "one 64 x 128 table": (2, [64, 128], [(0, 1)]),
    "1-D tables only": (64, [128] * 64, [(k,) for k in range(64)]),
    "unequal bins, scrambled requests": (9, [1, 64, 7, 0, 33, 128, 2, 64, 5],
                                         [(4, 7), (0,), (1, 5), (2, 8), (5,), (0, 1), (6, 7), (1, 2), (7,), (4, 5)]),
}


@pytest.mark.parametrize("teams", [1, 4])
@pytest.mark.parametrize("name", list(WPLAN_CASES))
def test_weighted_planner_invariants(planner, name, teams):
    d, bins, keep = WPLAN_CASES[name]
    keep = H.corner(bins) if keep is None else keep
    lines = planner(d, bins, keep, teams)
    head, _ = _parse(lines)
    if teams == 4 and max(H.sizes(keep, bins)) * 2 * 4 > 16384:
        assert int(head["plan"][0]) == 0          # a table past a wave's share: the call takes a workgroup per point
        return
    groups = _check_plan(lines, d, bins, keep, teams)
    if name == "one 90 x 90 table":
        assert len(groups) == 1 and groups[0]["head"][3] == 16200
    if name == "one 64 x 128 table":
        assert groups[0]["head"][3] == 16384
    if name == "d = 64 corner at 32 bins":
        assert len(keep) == 2080


def test_weighted_planner_reports_the_table_rules(planner):
    for d, bins, keep, status, words in ((2, [91, 91], [(0,), (0, 1)], _lib.DF_ERR_UNSUPPORTED, ("keep[1]", "8281", "8192")),
                                         (2, [128, 128], [(0, 1)], _lib.DF_ERR_UNSUPPORTED, ("keep[0]", "16384")),
                                         (3, [4, 5, 6], [(0,), (0,)], _lib.DF_ERR_INVALID, ("keep[1]",)),
                                         (3, [4, 5, 129], [(0,)], _lib.DF_ERR_UNSUPPORTED, ("bins[2]",)),
                                         (2, [91, 91], [(0, 1), (0, 1)], _lib.DF_ERR_INVALID, ("repeats",))):
        head, _ = _parse(planner(d, bins, keep, 1))
        assert int(head["check"][0]) == status and all(w in " ".join(head["message"]) for w in words), head
    head, _ = _parse(planner(3, [4, 5, 6], [(0, 1)], 1, n_points=(1 << 61) // 20))
    assert int(head["check"][0]) == _lib.DF_ERR_SHAPE
    head, _ = _parse(planner(3, [4, 5, 6], [(0, 1)], 1, n_points=(1 << 60) // 20 - 1))
    assert int(head["check"][0]) == _lib.DF_OK
