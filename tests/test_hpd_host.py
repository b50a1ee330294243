"""Host side of the calibration call (df_calib.hip), on CPU: df_flow_hpd_ranks is declared,
bound and exported at ABI 5; its argument errors come back before any device work, each with
a message naming the rule; the Python wrappers refuse bad arguments before the library is
touched; expected_coverage is the plain count of tests/hpd_ref.py."""
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
import hpd_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densityflows_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    m = re.search(r"^int\s+df_flow_hpd_ranks\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "df_flow_hpd_ranks is not declared in the header"
    assert len(m.group(1).split(",")) == 12
    res, args = _lib.SIGNATURES["df_flow_hpd_ranks"]
    assert res is C.c_int and len(args) == 12
    assert hasattr(lib, "df_flow_hpd_ranks"), "df_flow_hpd_ranks is not exported"
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", src)
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION
    assert hasattr(dfa.hip.HIPChain, "run_hpd_ranks")
    for name in ("hpd_levels", "expected_coverage"):
        assert name in flows.__all__ and hasattr(dfa, name)


def test_argument_errors_before_device_work():
    """No device exists here: every status below is returned by a check that stands before
    the first use of the handle (a non-null handle is a buffer that is never read)."""
    lib = _lib.load()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    null = C.c_void_p(0)
    out = C.c_void_p(C.addressof(C.create_string_buffer(8 * 16)))
    u = C.c_uint64

    def call(chain=fake, n_points=4, n_draws=8, chunk=0, rank=out):
        return lib.df_flow_hpd_ranks(chain, out, null, n_points, n_draws, chunk, u(1), u(0), rank, null, null, null)

    def message():
        return lib.df_last_error().decode("utf-8")

    assert call(chain=null) == _lib.DF_ERR_INVALID and "null chain" in message()
    assert call(rank=null) == _lib.DF_ERR_INVALID and "rank" in message()
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in message()
    assert call(chunk=-1) == _lib.DF_ERR_SHAPE and "chunk" in message()
    for bad in (0, -4, 6):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID, bad
        assert "multiple of 4" in message(), bad
    assert call(chunk=(1 << 24) + 1) == _lib.DF_ERR_UNSUPPORTED and "2^24" in message() and "chunk" in message()
    assert call(n_draws=(1 << 24) + 4) == _lib.DF_ERR_UNSUPPORTED and "2^24" in message() and "n_draws" in message()
    # the same rules hold for an empty call
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, rank=null) == _lib.DF_ERR_INVALID
    # an empty call with sound arguments runs nothing: the fake handle is never read
    assert call(n_points=0) == _lib.DF_OK
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        _lib.check(call(n_draws=6))
    with pytest.raises(_lib.UnsupportedError):
        _lib.check(call(chunk=(1 << 24) + 1))


def _flow():
    make, d, n = SPECS["readme"]
    spec = make(np.random.default_rng(0))
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, np.array([-1.0], np.float32),
                                                            np.array([3.0], np.float32)))


def test_python_argument_errors(monkeypatch):
    """Raised before the library is touched: Flow.hip (the only way to it) is never called."""
    flow = _flow()

    def no_device(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(dfa.Flow, "hip", no_device)
    x = np.zeros((5, 3, 2), np.float32)
    th = np.ones((1, 3, 2), np.float32)
    for bad in ((1.0, 2.0), (), None, np.ones((1, 3), np.float32), np.ones((2, 3, 2), np.float32)):
        with pytest.raises(AssertionError, match="dimensions θ"):
            dfa.hpd_levels(flow, x, bad, seed=1)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(5, dims"):
        dfa.hpd_levels(flow, np.zeros((4, 3, 2), np.float32), th, seed=1)
    for bad in (0, -4, 6, 1023):
        with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
            dfa.hpd_levels(flow, x, th, n_draws=bad, seed=1)
    with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
        dfa.hpd_levels(flow, x, th, chunk=(1 << 24) + 1, seed=1)
    with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
        dfa.hpd_levels(flow, x, th, n_draws=(1 << 24) + 4, seed=1)
    with pytest.raises(_lib.DimensionMismatch, match="chunk"):
        dfa.hpd_levels(flow, x, th, chunk=-4, seed=1)
    # sound arguments reach the library
    with pytest.raises(AssertionError, match="the library was touched"):
        dfa.hpd_levels(flow, x, (1.25,), n_draws=8, seed=1)


def test_ranks_reference():
    p = np.array([0.0, -np.inf, np.nan, 1.0, np.inf], np.float32)
    q = np.array([[0.0, 1.0, -1.0, np.nan], [-np.inf, 0.0, np.nan, np.inf], [0.0, 1.0, np.nan, np.inf],
                  [1.0, np.nextafter(np.float32(1), np.float32(2)), np.inf, 0.5], [np.inf, 0.0, 1e30, np.nan]],
                 np.float32)
    r = H.ranks(p, q)
    assert r.dtype == np.int32
    np.testing.assert_array_equal(r, [1, 2, 0, 2, 0])


@pytest.mark.parametrize("name", ["readme", "cfg2", "wide"])
def test_bracket_is_tight_for_the_oracle_alone(name):
    """The cap of tests/test_gpu_hpd.py::test_ranks_against_oracle, Σ(hi − lo) <= 0.01 · M · N,
    is a property of the lp distribution of these chains, points and θ, not of the Philox
    stream: the oracle alone meets it with numpy normal draws standing in for the device's."""
    make, d, n = SPECS[name]
    spec = make(np.random.default_rng(0))
    M, N = H.ORACLE_M, H.ORACLE_N
    x, th = _inputs(d, n, M)
    z64 = np.random.default_rng(9).standard_normal((d, M * N)).astype(np.float32).astype(np.float64)
    lp_p, lp_q = H.oracle_lp(spec, x, th, z64, N, np.full(n, -1.0, np.float32), np.full(n, 3.0, np.float32))
    lo, hi = H.bracket(lp_p, lp_q)
    print(f"{name}: oracle bracket share {np.sum(hi - lo) / (M * N):.5f}, lo {lo[:6]}, hi {hi[:6]}")
    assert np.all(lo <= hi) and np.sum(hi - lo) <= 0.01 * M * N


def test_expected_coverage():
    rng = np.random.default_rng(5)
    N = 64
    levels = rng.integers(0, N + 1, size=(7, 31)) / N        # multiples of 1/N, 0 and 1 included
    levels[0, :4] = [0.0, 1.0, 0.25, 0.5]                      # end points and exact grid values
    c, cov = dfa.expected_coverage(levels)
    rc, rcov = H.expected_coverage(levels)
    np.testing.assert_array_equal(c, np.linspace(0.0, 1.0, 101))
    np.testing.assert_array_equal(c, rc)
    np.testing.assert_array_equal(cov, rcov)
    assert cov[-1] == 1.0 and cov[0] == np.count_nonzero(levels == 0.0) / levels.size
    assert np.all(np.diff(cov) >= 0)
    # a grid of the caller's, its values exactly on levels: <= counts them
    grid = np.array([0.0, 1 / N, 0.25, 0.5, 1.0 - 1 / N, 1.0])
    c2, cov2 = dfa.expected_coverage(levels, grid)
    np.testing.assert_array_equal(c2, grid)
    np.testing.assert_array_equal(cov2, H.expected_coverage(levels, grid)[1])
    assert cov2[2] == np.count_nonzero(levels <= 0.25) / levels.size
    # one level on the grid value itself
    np.testing.assert_array_equal(dfa.expected_coverage([0.5], [0.49, 0.5, 0.51])[1], [0.0, 1.0, 1.0])
    with pytest.raises(_lib.ArgumentError, match="NaN"):
        dfa.expected_coverage([0.5, np.nan])
    assert "1 / n_draws" in dfa.expected_coverage.__doc__
