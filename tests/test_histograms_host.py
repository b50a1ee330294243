"""Host side of the histogram calls (df_hist.hip), on CPU: df_draw_histograms and
df_flow_point_histograms are declared, bound and exported at ABI 5; their argument errors come
back before any device work, in the documented order, each with a message naming the rule; the
Python wrappers refuse bad edges, bad keep and bad shapes before the library is touched; the
reference of tests/histogram_ref.py (np.histogram / np.histogram2d) agrees with a brute-force
loop on every edge case of the bin rule; and the host planner of the table groups
(df_hist_plan.cpp, printed by tests/hist_plan_check.cpp) keeps its invariants."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
from densityflows_amd.data import MetaData
from helpers import spec_to_element
from train_edge_cases import SPECS
import histogram_ref as H
import test_plan_fingerprint as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densityflows_hip.h")).read(), flags=re.S)


def test_calls_declared_bound_and_exported():
    src = _header()
    lib = _lib.load()
    for name, count in (("df_draw_histograms", 10), ("df_flow_point_histograms", 14)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == count
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == count
        assert hasattr(lib, name), f"{name} is not exported"
    for macro, value in (("DF_HIST_MAX_BINS", dfa.HIST_MAX_BINS), ("DF_HIST_MAX_TABLES", dfa.HIST_MAX_TABLES),
                         ("DF_HIST_SPLIT_DRAWS", dfa.HIST_SPLIT_DRAWS)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", src)
        assert m and int(m.group(1)) == value, macro
    assert dfa.HIST_MAX_BINS == 128 and dfa.HIST_MAX_TABLES == 2080 == 64 + 64 * 63 // 2
    assert dfa.HIST_SPLIT_DRAWS % 256 == 0 and dfa.HIST_SPLIT_DRAWS > 256
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", src)
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION
    assert hasattr(dfa.hip.HIPChain, "run_point_histograms") and hasattr(dfa.hip.HIPChain, "run_draw_histograms")
    assert hasattr(dfa.hip, "run_draw_histograms")
    for name in ("histogram_edges", "draw_histograms", "posterior_histograms", "PointHistograms", "HIST_MAX_BINS",
                 "HIST_MAX_TABLES", "HIST_SPLIT_DRAWS"):
        assert name in flows.__all__ and hasattr(dfa, name)


def _i32(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def _message(lib):
    return lib.df_last_error().decode("utf-8")


CORNER3 = _i32(0, -1, 1, -1, 2, -1, 0, 1, 0, 2, 1, 2)        # d = 3: 6 tables


def test_draw_histograms_argument_errors_before_device_work():
    """No device exists here: every status below is returned before anything is launched.  The
    pointers that stand for device memory are host buffers that are never read."""
    lib = _lib.load()
    buf = C.create_string_buffer(512)
    base = (C.addressof(buf) + 15) & ~15
    xs, out, ed, null = C.c_void_p(base), C.c_void_p(base + 64), C.c_void_p(base + 128), C.c_void_p(0)

    def call(xs=xs, d=3, n_points=4, n_draws=8, edges=ed, bins=_i32(4, 5, 6), keep=CORNER3, n_tables=6, out=out):
        return lib.df_draw_histograms(xs, d, n_points, n_draws, edges, bins, keep, n_tables, out, null)

    # 1. d
    for bad in (0, -1, 65):
        assert call(d=bad) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(lib), bad
    # 2. n_points
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message(lib)
    # 3. n_draws
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib), bad
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib)
    # 4. pointers
    assert call(xs=null) == _lib.DF_ERR_INVALID and "null xs or counts_out" in _message(lib)
    assert call(out=null) == _lib.DF_ERR_INVALID and "null xs or counts_out" in _message(lib)
    assert call(edges=null) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    assert call(bins=None) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    assert call(keep=None) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    for off in (4, 8, 12):
        assert call(xs=C.c_void_p(base + off)) == _lib.DF_ERR_INVALID and "16-byte" in _message(lib), off
    # 5. n_tables
    for bad in (0, -1, 2081):
        assert call(n_tables=bad) == _lib.DF_ERR_UNSUPPORTED and "n_tables" in _message(lib), bad
    # 6. bins
    assert call(bins=_i32(4, -1, 6)) == _lib.DF_ERR_INVALID and "bins[1]" in _message(lib)
    assert call(bins=_i32(4, 5, 129)) == _lib.DF_ERR_UNSUPPORTED and "bins[2]" in _message(lib)
    # 7. requests
    one = lambda a, b: dict(keep=_i32(0, -1, a, b), n_tables=2)
    assert call(**one(3, -1)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib) and "first" in _message(lib)
    assert call(**one(-1, -1)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib)
    assert call(**one(1, 1)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib) and "second" in _message(lib)
    assert call(**one(2, 1)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib)
    assert call(**one(1, 3)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib)
    assert call(**one(1, -2)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib)
    assert call(**one(0, -1)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib) and "repeats" in _message(lib)
    assert call(keep=_i32(0, 1, 1, 2, 0, 1), n_tables=3) == _lib.DF_ERR_INVALID and "keep[2]" in _message(lib)
    assert call(bins=_i32(4, 0, 6), **one(1, -1)) == _lib.DF_ERR_INVALID and "without bins" in _message(lib)
    assert call(bins=_i32(4, 0, 6), **one(1, 2)) == _lib.DF_ERR_INVALID and "keep[1]" in _message(lib)
    assert call(bins=_i32(4, 5, 0), **one(1, 2)) == _lib.DF_ERR_INVALID and "without bins" in _message(lib)
    # 8. T · n_points past int64 (T = 4 + 5 + 6 + 20 + 24 + 30 = 89)
    assert call(n_points=(1 << 62) // 89) == _lib.DF_ERR_SHAPE and "int64" in _message(lib)
    # the order of the checks: each rule before the next
    assert call(d=0, n_points=-1) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(lib)
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, xs=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib)
    assert call(xs=null, n_tables=0) == _lib.DF_ERR_INVALID and "null" in _message(lib)
    assert call(n_tables=0, bins=_i32(4, -1, 6)) == _lib.DF_ERR_UNSUPPORTED and "n_tables" in _message(lib)
    assert call(bins=_i32(4, 5, 129), **one(3, -1)) == _lib.DF_ERR_UNSUPPORTED and "bins[2]" in _message(lib)
    assert call(n_points=(1 << 62) // 89, **one(0, -1)) == _lib.DF_ERR_INVALID and "repeats" in _message(lib)
    # 9. the same rules hold for an empty call
    assert call(n_points=0, d=0) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, xs=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, out=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, edges=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_tables=0) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, bins=_i32(4, 5, 129)) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, **one(0, -1)) == _lib.DF_ERR_INVALID
    # an empty call with sound arguments launches nothing: also the full corner at d = 64
    assert call(n_points=0) == _lib.DF_OK
    k64 = [v for K in H.corner([4] * 64) for v in (K + (-1,))[:2]]
    assert len(k64) == 2 * 2080
    assert call(n_points=0, d=64, bins=_i32(*([4] * 64)), keep=_i32(*k64), n_tables=2080) == _lib.DF_OK
    assert call(n_points=0, d=2, bins=_i32(128, 128), keep=_i32(0, 1), n_tables=1) == _lib.DF_OK
    with pytest.raises(_lib.ArgumentError, match=r"keep\[1\]"):
        _lib.check(call(**one(0, -1)))
    with pytest.raises(_lib.UnsupportedError, match="n_tables"):
        _lib.check(call(n_tables=2081))
    with pytest.raises(_lib.DimensionMismatch):
        _lib.check(call(n_points=-3))


def test_point_histograms_argument_errors_before_device_work():
    """The rules of df_flow_point_stats in its order and with its messages, then the outputs, then
    the table arrays and their count: each returned before the handle is read (a non-null handle
    is a buffer that is never read).  The rules on bins and requests need the chain's d and are
    df_draw_histograms' own code (above)."""
    lib = _lib.load()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    null = C.c_void_p(0)
    out = C.c_void_p(C.addressof(C.create_string_buffer(8 * 16)))
    u = C.c_uint64

    def call(chain=fake, n_points=4, n_draws=8, chunk=0, edges=out, bins=_i32(4, 5, 6), keep=CORNER3, n_tables=0,
             counts=out, draws=null):
        return lib.df_flow_point_histograms(chain, null, n_points, n_draws, chunk, u(1), u(0), edges, bins, keep,
                                            n_tables, counts, draws, null)

    assert call(chain=null) == _lib.DF_ERR_INVALID and "null chain" in _message(lib)
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message(lib)
    assert call(chunk=-1) == _lib.DF_ERR_SHAPE and "chunk" in _message(lib)
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID, bad
        assert "multiple of 4" in _message(lib) and "Philox" in _message(lib), bad
    assert call(chunk=(1 << 24) + 1) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib) and "chunk" in _message(lib)
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message(lib) and "n_draws" in _message(lib)
    assert call(counts=null) == _lib.DF_ERR_INVALID and "no output" in _message(lib)
    assert call(edges=null) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    assert call(bins=None) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    assert call(keep=None) == _lib.DF_ERR_INVALID and "null edges, bins or keep" in _message(lib)
    for bad in (0, -1, 2081):
        assert call(n_tables=bad) == _lib.DF_ERR_UNSUPPORTED and "n_tables" in _message(lib), bad
    # the order: the point count before n_draws, n_draws before the outputs, the outputs before the tables
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, counts=null) == _lib.DF_ERR_INVALID and "multiple of 4" in _message(lib)
    assert call(counts=null, edges=null) == _lib.DF_ERR_INVALID and "no output" in _message(lib)
    assert call(edges=null, n_tables=2081) == _lib.DF_ERR_INVALID and "null edges" in _message(lib)
    # the same rules hold for an empty call
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, counts=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, keep=None) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_tables=2081) == _lib.DF_ERR_UNSUPPORTED
    # the draws alone: edges, bins, keep and n_tables are not looked at, the handle is never read
    assert call(n_points=0, counts=null, draws=out) == _lib.DF_OK
    assert call(n_points=0, counts=null, draws=out, edges=null, bins=None, keep=None, n_tables=-7) == _lib.DF_OK
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        _lib.check(call(n_draws=6))
    with pytest.raises(_lib.UnsupportedError):
        _lib.check(call(chunk=(1 << 24) + 1))


# ---------------------------------------------------------------------------
# the reference against the brute-force loop
# ---------------------------------------------------------------------------

def _edge_sets():
    f = np.float32
    return {
        "uniform": np.linspace(-2, 2, 9).astype(f),
        "L = 1": np.array([-0.5, 0.75], f),
        "L = 128": np.linspace(-3, 3, 129).astype(f),
        "unequal widths": np.array([-4, -1, -0.875, 0, 1e-3, 0.5, 3], f),
        "edge at +0": np.array([-1, 0.0, 1], f),
        "first edge +0": np.array([0.0, 0.5, 2], f),
        "infinite outer edges": np.array([-np.inf, -1, 0.25, np.inf], f),
        "infinite last edge": np.array([-1, 0, np.inf], f),
        "neighbouring floats": np.array([1.0, np.nextafter(f(1), f(2)), np.nextafter(np.nextafter(f(1), f(2)), f(2))], f),
    }


def _probe_values(e):
    lo, hi = H.ulp_neighbours(e)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001], np.uint32).view(np.float32)
    v = np.concatenate([e, lo, hi, nan, np.array([np.inf, -np.inf, 0.0, -0.0, 3e38, -3e38, 1e-45, -1e-45], np.float32),
                        np.random.default_rng(len(e)).standard_normal(61).astype(np.float32)])
    return v[:len(v) // 4 * 4]


@pytest.mark.parametrize("name", list(_edge_sets()))
def test_reference_agrees_with_brute_force(name):
    """Draws exactly on every edge, on the last edge, one ulp either side of an edge, below the
    first and above the last edge, NaN, ±inf and −0 against +0: numpy's counts are the rule's."""
    e = _edge_sets()[name]
    other = _edge_sets()["unequal widths"]
    v = _probe_values(e)
    rng = np.random.default_rng(3)
    w = rng.choice(_probe_values(other), v.size)
    q = np.stack([np.stack([v, w], axis=1), np.stack([rng.permutation(v), rng.permutation(w)], axis=1)])
    edges = [e, other]
    keep = [(1,), (0,), (0, 1)]
    ref = H.blocks(q, edges, keep)
    np.testing.assert_array_equal(ref, H.blocks_brute(q, edges, keep))
    np.testing.assert_array_equal(ref, H.blocks_indexed(q, edges, keep))
    L = len(e) - 1
    # the rule, stated once more on single values
    assert H.bin_of(e[0], e) == 0 and H.bin_of(e[L], e) == L - 1
    below = np.nextafter(e[0], np.float32(-np.inf))
    if np.isfinite(e[0]):
        assert H.bin_of(below, e) == -1
    if np.isfinite(e[L]):
        assert H.bin_of(np.nextafter(e[L], np.float32(np.inf)), e) == -1
    else:
        assert H.bin_of(np.inf, e) == L - 1                      # an infinite draw on an infinite last edge
    assert H.bin_of(np.nan, e) == -1
    if name == "edge at +0":
        assert H.bin_of(np.float32(-0.0), e) == 1 and H.bin_of(np.float32(0.0), e) == 1
    if name == "first edge +0":
        assert H.bin_of(np.float32(-0.0), e) == 0
    # sums: the inside counts
    inside0 = sum(H.bin_of(x, e) >= 0 for x in q[0, :, 0])
    assert ref[0, len(other) - 1:len(other) - 1 + L].sum() == inside0


def test_reference_layout():
    """Request order and i_a + L_a·i_b."""
    rng = np.random.default_rng(8)
    q = rng.standard_normal((2, 40, 3)).astype(np.float32)
    edges = [np.linspace(-2, 2, 4).astype(np.float32), None, np.linspace(-1, 1, 6).astype(np.float32)]
    np.testing.assert_array_equal(H.bins_of(edges), [3, 0, 5])
    assert H.corner(H.bins_of(edges)) == [(0,), (2,), (0, 2)]
    keep = [(0, 2), (2,)]
    b = H.blocks(q, edges, keep)
    assert b.shape == (2, 15 + 5) and b.dtype == np.int32
    h2, _, _ = np.histogram2d(q[1, :, 0], q[1, :, 2], (edges[0], edges[2]))
    for ia in range(3):
        for ib in range(5):
            assert b[1, ia + 3 * ib] == h2[ia, ib]
    np.testing.assert_array_equal(b[1, 15:], np.histogram(q[1, :, 2], edges[2])[0])
    np.testing.assert_array_equal(H.flat_edges(edges), np.concatenate([edges[0], edges[2]]))
    np.testing.assert_array_equal(b, H.blocks_indexed(q, edges, keep))


def test_planted_draws_and_the_indexed_reference():
    """The draws the GPU tests plant (every edge's bits, its ulp neighbours, NaN, ±inf, ±0, far
    outside) under the three references."""
    rng = np.random.default_rng(9)
    d = 5
    edges = [np.linspace(-2 - 0.25 * k, 2 + 0.5 * k, 9).astype(np.float32) for k in range(d)]
    edges[3] = None
    q = H.plant(rng.standard_normal((3, 68, d)).astype(np.float32), edges, rng)
    assert np.isnan(q).any() and np.isinf(q).any() and (q == edges[0][4]).any()
    keep = H.corner(H.bins_of(edges))
    ref = H.blocks(q, edges, keep)
    np.testing.assert_array_equal(ref, H.blocks_brute(q, edges, keep))
    np.testing.assert_array_equal(ref, H.blocks_indexed(q, edges, keep))
    assert ref.sum() < 3 * 68 * len(keep)                     # some draws are outside


# ---------------------------------------------------------------------------
# the Python wrappers
# ---------------------------------------------------------------------------

def test_histogram_edges():
    ev, bins = dfa.histogram_edges([None, (-1.0, 1.0, 4), [0, 1, 3], np.array([-np.inf, 0, np.inf])], 4)
    assert ev[0] is None and bins.dtype == np.int32
    np.testing.assert_array_equal(bins, [0, 4, 2, 2])
    assert all(v.dtype == np.float32 for v in ev[1:])
    np.testing.assert_array_equal(ev[1], np.linspace(-1.0, 1.0, 5).astype(np.float32))
    np.testing.assert_array_equal(ev[2], [0, 1, 3])
    # a triple is np.linspace in float64, rounded once
    ev, _ = dfa.histogram_edges([(0.1, 0.7, 7)], 1)
    np.testing.assert_array_equal(ev[0], np.linspace(0.1, 0.7, 8).astype(np.float32))
    dfa.histogram_edges([np.linspace(0, 1, 129)], 1)                     # 128 bins
    dfa.histogram_edges([(0.0, 1.0, 128)], 1)
    for bad, what in (([np.linspace(0, 1, 130)], "more than 129"), ([[1.0]], "fewer than 2"), ([[]], "fewer than 2"),
                      ([[0, np.nan, 1]], "NaN"), ([[0, 1, 1]], "strictly increasing"), ([[0, 2, 1]], "strictly increasing"),
                      ([[1.0, 1.0 + 1e-9]], "strictly increasing"),       # equal after rounding to Float32
                      ([(0.0, 1.0, 129)], "nbins"), ([(0.0, 1.0, 0)], "nbins"), ([(1.0, 1.0, 4)], "strictly increasing"),
                      ([(0.0, np.nan, 4)], "NaN"), ([np.zeros((2, 2))], "vector")):
        with pytest.raises(_lib.ArgumentError, match=what) as err:
            dfa.histogram_edges([None] + bad, 2)
        assert "dimension 1" in str(err.value), bad
    with pytest.raises(_lib.DimensionMismatch, match="d = 3"):
        dfa.histogram_edges([None, None], 3)


def _flow(name="readme"):
    make, d, n = SPECS[name]
    spec = make(np.random.default_rng(0))
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, np.full(n, -1.0, np.float32),
                                                            np.full(n, 3.0, np.float32)))


def test_python_argument_errors(monkeypatch):
    """Raised before the library is touched: Flow.hip, and the module-level counting call (the
    only ways to it) are never reached."""
    flow = _flow()

    def no_device(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(dfa.Flow, "hip", no_device)
    monkeypatch.setattr(dfa.hip, "run_draw_histograms", no_device)
    th = np.ones((1, 3, 2), np.float32)
    e5 = [(-2.0, 2.0, 8)] * 5
    fn = lambda t=th, edges=e5, **k: dfa.posterior_histograms(flow, t, edges=edges, seed=1, **k)
    for bad in ((1.0, 2.0), (), None, np.ones((1, 3), np.float32)[:0].reshape(0, 3), np.ones((2, 3, 2), np.float32)):
        with pytest.raises(AssertionError, match="dimensions θ"):
            fn(bad)
    for bad in (0, -4, 6, 1023):
        with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
            fn(n_draws=bad)
    with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
        fn(chunk=(1 << 24) + 1)
    with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
        fn(n_draws=(1 << 24) + 4)
    with pytest.raises(_lib.DimensionMismatch, match="chunk"):
        fn(chunk=-4)
    with pytest.raises(_lib.ArgumentError, match="dims="):
        fn((1.25,))
    with pytest.raises(_lib.ArgumentError, match="needs edges"):
        fn(edges=None)
    with pytest.raises(_lib.DimensionMismatch, match="d = 5"):
        fn(edges=e5[:4])
    with pytest.raises(_lib.ArgumentError, match="dimension 2"):
        fn(edges=e5[:2] + [[0, 0]] + e5[3:])
    for bad, exc in (([(0, 5)], _lib.ArgumentError), ([(1, 1)], _lib.ArgumentError), ([(-1,)], _lib.ArgumentError),
                     ([()], _lib.ArgumentError), ([], _lib.ArgumentError), ([(0, 1, 2)], _lib.UnsupportedError)):
        with pytest.raises(exc):
            fn(keep=bad)
    with pytest.raises(_lib.ArgumentError, match="without edges"):
        fn(edges=[None] + e5[1:], keep=[(0, 1)])
    with pytest.raises(_lib.ArgumentError, match="no histogram tables"):
        fn(edges=[None] * 5)
    # sound arguments reach the library
    with pytest.raises(AssertionError, match="the library was touched"):
        fn(n_draws=8)
    with pytest.raises(AssertionError, match="the library was touched"):
        fn((1.25,), n_draws=8, dims=(3, 2), keep=[(3, 1), 2, (1, 3)])
    # draw_histograms
    q = np.zeros((3, 8, 5), np.float32)
    with pytest.raises(_lib.ArgumentError, match="Float32"):
        dfa.draw_histograms(q.astype(np.float64), e5)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(M, N, d\)"):
        dfa.draw_histograms(q[0], e5)
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        dfa.draw_histograms(q[:, :6], e5)
    with pytest.raises(_lib.ArgumentError, match="1 .. 64"):
        dfa.draw_histograms(np.zeros((1, 8, 65), np.float32), [None] * 65)
    with pytest.raises(_lib.DimensionMismatch, match="d = 5"):
        dfa.draw_histograms(q, e5[:3])
    with pytest.raises(_lib.ArgumentError, match="dimension 0"):
        dfa.draw_histograms(q, [[3, 2, 1]] + e5[1:])
    with pytest.raises(_lib.ArgumentError):
        dfa.draw_histograms(q, e5, keep=[(4, 5)])
    with pytest.raises(_lib.UnsupportedError):
        dfa.draw_histograms(q, e5, keep=[(0, 1, 2)])


def test_requests_are_merged_and_sorted():
    bins = np.array([4, 0, 3, 2], np.int32)
    assert flows._histogram_requests(None, bins) == [(0,), (2,), (3,), (0, 2), (0, 3), (2, 3)] == H.corner(bins)
    assert flows._histogram_requests([(3, 0), 2, (0, 3), (2,), np.int64(0)], bins) == [(0,), (2,), (0, 3)]


def test_point_histograms_object():
    edges = [np.array([-1, 0, 2], np.float32), np.array([0, 1, 2, 4], np.float32)]
    c1 = np.array([[3, 5], [0, 8]], np.int32)
    c2 = np.arange(12, dtype=np.int32).reshape(2, 2, 3)
    ph = dfa.PointHistograms({(0,): c1, (0, 1): c2}, edges, 16, (2,))
    np.testing.assert_array_equal(ph.inside(0), [8, 8])
    np.testing.assert_array_equal(ph.inside((0, 1)), [15, 51])
    np.testing.assert_array_equal(ph.pooled((0,)), [3, 13])
    assert ph.pooled((0, 1)).dtype == np.int64 and ph.pooled((0, 1)).shape == (2, 3)
    den = ph.density(0)
    assert den.dtype == np.float64
    np.testing.assert_allclose((den * np.diff(edges[0])).sum(axis=1), ph.inside(0) / 16, rtol=1e-15)
    den2 = ph.density((0, 1))
    area = np.diff(edges[0])[:, None] * np.diff(edges[1])[None, :]
    np.testing.assert_allclose((den2 * area).sum(axis=(1, 2)), ph.inside((0, 1)) / 16, rtol=1e-15)
    assert "tables=2" in repr(ph)


# ---------------------------------------------------------------------------
# the host planner of the table groups
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("hist_plan"))
    exe = PF.compile_program(os.path.join(PF.CSRC, "df_hist_plan.cpp"), os.path.join(work, "hist_plan_check"),
                             program="hist_plan_check.cpp")
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
    """The invariants: every requested table in exactly one group; every group within the LDS
    budget and the descriptor's capacity; the offsets tile [0, T) in request order; the edges
    and the tables of a group tile its LDS parts."""
    head, groups = _parse(lines)
    assert int(head["check"][0]) == 0, head
    T = sum(H.sizes(keep, bins))
    assert int(head["check"][1]) == T and int(head["plan"][2]) == T
    assert int(head["plan"][0]) == 1 and int(head["plan"][1]) == len(groups) >= 1
    lds_words, table_words, max_dims, max_tables = (int(v) for v in head["budget"])
    assert lds_words * 4 * 2 <= 160 * 1024 and table_words * 4 == 64 * 1024
    src = np.concatenate([[0], np.cumsum([b + 1 if b > 0 else 0 for b in bins])])
    want_off = dict(zip([(K[0], K[1] if len(K) == 2 else -1) for K in keep], np.concatenate([[0], np.cumsum(H.sizes(keep, bins))])))
    seen = {}
    for g in groups:
        n_dims, n_tables, edge_words, tw, lds = g["head"]
        assert 1 <= n_dims == len(g["dims"]) <= max_dims and 1 <= n_tables == len(g["tables"]) <= max_tables
        assert lds <= lds_words and teams * tw <= table_words and tw % 4 == 0
        assert lds == 64 + (edge_words + 3) // 4 * 4 + teams * tw + 4 * 64 * (n_dims | 1)
        at = 0
        mine = set()
        for dim, L, esrc, elds in g["dims"]:
            assert 0 <= dim < d and L == bins[dim] > 0 and esrc == src[dim] and elds == at and dim not in mine
            mine.add(dim)
            at += L + 1
        assert at == edge_words
        at = 0
        for a, b, out_off, lds_off in g["tables"]:
            assert a in mine and (b == -1 or (b in mine and a < b))
            assert (a, b) not in seen, "a table in two groups"
            seen[(a, b)] = out_off
            assert out_off == want_off[(a, b)] and lds_off == at
            at += bins[a] * (bins[b] if b >= 0 else 1)
        assert at <= tw < at + 4
    assert set(seen) == set(want_off), "a requested table in no group"
    # the offsets tile [0, T) without overlap
    spans = sorted((off, off + bins[a] * (bins[b] if b >= 0 else 1)) for (a, b), off in seen.items())
    assert spans[0][0] == 0 and spans[-1][1] == T
    assert all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
    return groups


PLAN_CASES = {
    "d = 5 corner at 32 bins": (5, [32] * 5, None),
    "d = 32 corner at 32 bins": (32, [32] * 32, None),
    "d = 64 corner at 4 bins": (64, [4] * 64, None),
    "one 128 x 128 table": (3, [128, 0, 128], [(0, 2)]),
    "1-D tables only": (64, [128] * 64, [(k,) for k in range(64)]),
    "unequal bins, scrambled requests": (9, [1, 128, 7, 0, 33, 128, 2, 64, 5],
                                         [(4, 7), (0,), (1, 5), (2, 8), (5,), (0, 1), (6, 7), (1, 2), (7,), (4, 5)]),
    "d = 61 corner at 8 bins": (61, [8] * 61, None),
}


@pytest.mark.parametrize("teams", [1, 4])
@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_planner_invariants(planner, name, teams):
    d, bins, keep = PLAN_CASES[name]
    keep = H.corner(bins) if keep is None else keep
    lines = planner(d, bins, keep, teams)
    head, _ = _parse(lines)
    if teams == 4 and max(H.sizes(keep, bins)) * 4 > 16384:
        assert int(head["plan"][0]) == 0          # a table past a wave's share: the call takes a workgroup per point
        return
    groups = _check_plan(lines, d, bins, keep, teams)
    if name == "d = 32 corner at 32 bins":
        assert len(groups) >= 2
        assert len(keep) == 528
    if name == "d = 64 corner at 4 bins":
        assert len(keep) == 2080
    if name == "one 128 x 128 table":
        assert len(groups) == 1 and groups[0]["head"][3] == 16384
    if name == "d = 5 corner at 32 bins" and teams == 1:
        assert len(groups) == 1                   # 15 tables: 5·32 + 10·1024 words
    print(f"{name}, {teams} team(s): {len(keep)} tables in {len(groups)} groups, "
          f"{sum(len(g['dims']) for g in groups)} bin searches per draw")


def test_planner_reports_the_table_rules(planner):
    """hist_check_tables is the code behind rules 5-8 of both calls."""
    for d, bins, keep, status, word in ((3, [4, 5, 6], [(0,), (0,)], _lib.DF_ERR_INVALID, "keep[1]"),
                                        (3, [4, 5, 129], [(0,)], _lib.DF_ERR_UNSUPPORTED, "bins[2]"),
                                        (3, [4, -5, 6], [(0,)], _lib.DF_ERR_INVALID, "bins[1]"),
                                        (3, [4, 0, 6], [(1, 2)], _lib.DF_ERR_INVALID, "keep[0]")):
        head, _ = _parse(planner(d, bins, keep, 1))
        assert int(head["check"][0]) == status and word in " ".join(head["message"])
    head, _ = _parse(planner(3, [4, 5, 6], [(0, 1)], 1, n_points=(1 << 62) // 20))
    assert int(head["check"][0]) == _lib.DF_ERR_SHAPE
