"""Grid logpdf on the CPU: the entry point is declared, bound and exported; the numpy
enumerator the GPU tests materialise grids with is pinned on a literal; and on every
grid tests/test_gpu_grid.py evaluates the oracle's own fp32 arithmetic keeps the 1e-5
criterion against fp64 with room to spare."""
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
import grid_cases as G
from helpers import close
from oracle import flow_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_signatures_bind_the_grid_call():
    src = open(os.path.join(ROOT, "include", "densityflows_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+df_flow_logpdf_grid\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "include/densityflows_hip.h does not declare df_flow_logpdf_grid"
    assert len(m.group(1).split(",")) == 8
    res, args = _lib.SIGNATURES["df_flow_logpdf_grid"]
    assert len(args) == 8
    assert hasattr(_lib.load(), "df_flow_logpdf_grid")
    assert _lib.ABI_VERSION == 5 and "#define DF_ABI_VERSION 5" in src


def test_null_arguments_are_rejected_without_a_device():
    import ctypes as C

    lib = _lib.load()
    lens = (C.c_int64 * 2)(2, 3)
    assert lib.df_flow_logpdf_grid(None, None, lens, 0, 0, None, 0, None) == _lib.DF_ERR_INVALID
    assert b"null chain" in lib.df_last_error()
    assert lib.df_theta_broadcast(None, None, 2, -1, None) == _lib.DF_ERR_SHAPE
    assert lib.df_theta_broadcast(None, None, 2, 0, None) == _lib.DF_OK


def test_logpdf_grid_is_exported():
    assert dfa.logpdf_grid is flows.logpdf_grid
    assert "logpdf_grid" in flows.__all__


def test_point_enumerator_on_a_literal():
    pts = G.grid_points([np.array([1, 2], np.float32), np.array([10, 20, 30], np.float32)])
    want = np.array([[1, 10], [2, 10], [1, 20], [2, 20], [1, 30], [2, 30]], np.float32).T
    assert pts.dtype == np.float32 and np.array_equal(pts, want)
    # a window is a slice of the whole; the order is Fortran order of the (2, 3) result
    assert np.array_equal(G.grid_points([[1, 2], [10, 20, 30]], 1, 4), want[:, 1:5])
    i, j = np.unravel_index(np.arange(6), (2, 3), order="F")
    assert np.array_equal(pts[0], np.array([1, 2], np.float32)[i])
    assert np.array_equal(pts[1], np.array([10, 20, 30], np.float32)[j])


def test_big_window_decode_is_64_bit():
    """The 2³⁵-point grid's window starts past 2³³: every axis index of its first point,
    from the digits of `first` in base 128."""
    axes = [np.arange(G.BIG_LEN, dtype=np.float32) + 1000 * k for k in range(5)]
    pts = G.grid_points(axes, G.BIG_FIRST, 3)
    digits = [(G.BIG_FIRST // 128**k) % 128 for k in range(5)]
    assert digits == [5, 0, 0, 0, 32]
    assert pts[:, 0].tolist() == [1000 * k + dg for k, dg in enumerate(digits)]
    assert pts[0].tolist() == [5, 6, 7]


@pytest.mark.parametrize("gid,args", G.all_grids(), ids=[g[0] for g in G.all_grids()])
def test_grid_fp32_oracle(gid, args):
    """As test_oracle.py::test_edge_cases_fp32_oracle: on each grid the GPU tests use, the
    oracle's fp32 logpdf against its fp64 under close(·, 1e-5) has a violation ratio of at
    most 0.5 (measured: at most 0.0074), so the GPU tests' tolerance is attainable."""
    D = G.grid_data(*args)
    assert np.all(np.isfinite(D["lp"]))
    lp32 = O.flow_logpdf(D["spec"], D["x"], D["th"], np.float32)
    r = close(lp32, D["lp"], 1e-5)[1]
    print(f"GRID {gid}: {D['x'].shape[1]} points, fp32 oracle violation ratio {r:.4f}")
    assert r <= 0.5, f"{gid}: fp32 oracle violation ratio {r}"
