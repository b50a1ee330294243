"""Marginal tables on the CPU: df_flow_pdf_marginals is declared, bound and exported; what it
can refuse without a device it refuses; trapezoid_weights is numpy.trapz; and the numpy
reference the GPU tests compare with (tests/marginal_ref.py) is pinned on a brute-force loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
import grid_cases as G
import marginal_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_signatures_bind_the_marginal_call():
    src = open(os.path.join(ROOT, "include", "densityflows_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+df_flow_pdf_marginals\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "include/densityflows_hip.h does not declare df_flow_pdf_marginals"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 11
    res, args = _lib.SIGNATURES["df_flow_pdf_marginals"]
    assert res is C.c_int and len(args) == 11
    want = {"int64_t": C.c_int64, "int32_t": C.c_int32, "const int64_t*": C.POINTER(C.c_int64),
            "const int32_t*": C.POINTER(C.c_int32)}
    for p, a in zip(params, args):
        ctype = p.rsplit(" ", 1)[0]
        assert a is want.get(ctype, C.c_void_p), (p, a)       # every other pointer: a device address or a handle
    assert hasattr(_lib.load(), "df_flow_pdf_marginals")
    assert _lib.ABI_VERSION == 5 and "#define DF_ABI_VERSION 5" in src


def test_null_arguments_are_rejected_without_a_device():
    lib = _lib.load()
    lens = (C.c_int64 * 2)(2, 3)
    keep = (C.c_int32 * 2)(0, -1)
    # a null chain, with nothing else and with lens only: the lengths cannot be judged
    # without the chain's d + n, so both are the null chain's error
    assert lib.df_flow_pdf_marginals(None, None, None, None, 0, 0, None, 0, None, 0, None) == _lib.DF_ERR_INVALID
    assert b"null chain" in lib.df_last_error()
    assert lib.df_flow_pdf_marginals(None, None, None, lens, 0, 0, keep, 1, None, 0, None) == _lib.DF_ERR_INVALID
    assert b"null chain" in lib.df_last_error()
    assert lib.df_flow_pdf_marginals(None, None, None, lens, 0, -1, None, 200, None, -1, None) == _lib.DF_ERR_INVALID


def test_pdf_marginals_is_exported():
    assert dfa.pdf_marginals is flows.pdf_marginals and dfa.trapezoid_weights is flows.trapezoid_weights
    assert "pdf_marginals" in flows.__all__ and "trapezoid_weights" in flows.__all__


def test_request_lists():
    lens = (3, 1, 5, 2, 7, 4)
    corner = flows._marginal_requests(None, lens, 5)        # x axes of more than one value only
    assert corner == [(), (0,), (2,), (3,), (4,), (0, 2), (0, 3), (0, 4), (2, 3), (2, 4), (3, 4)]
    assert flows._marginal_requests([(4, 0), (5,), (), (0, 4), 2], lens, 5) == [(), (2,), (5,), (0, 4)]
    with pytest.raises(_lib.UnsupportedError):
        flows._marginal_requests([(0, 1, 2)], lens, 5)
    with pytest.raises(_lib.UnsupportedError):
        flows._marginal_requests(M.all_requests(16), (2,) * 16, 16)      # 137 tables
    for bad in ((6,), (-1,), (2, 2)):
        with pytest.raises(_lib.ArgumentError):
            flows._marginal_requests([bad], lens, 5)


def test_trapezoid_weights_are_numpy_trapz():
    """Σ w·f against numpy.trapz within 1e-15 relative on non-uniform axes.  All terms are
    positive; the two sums round differently, by a few units of 1.1e-16 for the short axes.
    The 41-point axis and its integrand are multiples of 1/8 and 1/16, on which both sums
    are exact."""
    trapz = getattr(np, "trapezoid", None) or np.trapz             # numpy 2 renamed it
    rng = np.random.default_rng(7)
    cases = []
    for L in (2, 3, 8):
        x = np.sort(rng.normal(size=L)).astype(np.float32)
        x += np.arange(L, dtype=np.float32) * np.float32(1e-3)           # strictly increasing, non-uniform
        cases.append((x, np.exp(-x.astype(np.float64)**2) + 0.25))
    cases.append((np.cumsum(rng.integers(1, 9, size=41)).astype(np.float32) / 8, rng.integers(1, 64, size=41) / 16.0))
    for x, f in cases:
        L = x.size
        assert np.all(np.diff(x) > 0) and (L == 2 or len(set(np.diff(x).tolist())) > 1)
        w = dfa.trapezoid_weights(x)
        assert w.dtype == np.float64 and w.shape == (L,) and np.all(w > 0)
        want = trapz(f, x.astype(np.float64))
        print(f"TRAPZ L={L}: relative difference {abs(w @ f - want) / abs(want):.3g}")
        assert abs(w @ f - want) <= 1e-15 * abs(want), (L, w @ f, want)
    assert dfa.trapezoid_weights([0.3]).tolist() == [1.0]
    assert dfa.trapezoid_weights([]).shape == (0,)
    assert dfa.trapezoid_weights([1.0, 3.0, 4.0]).tolist() == [1.0, 1.5, 0.5]
    with pytest.raises(_lib.DimensionMismatch):
        dfa.trapezoid_weights(np.zeros((2, 2)))


def _brute(values, axes, weights, keep, first=0):
    """One Python loop over the points grid_points enumerates, indices found by value."""
    lens = [len(a) for a in axes]
    pts = G.grid_points(axes, first, len(values))
    out = np.zeros(M.table_shape(lens, keep), np.float64)
    for p in range(len(values)):
        idx = [int(np.nonzero(np.asarray(a, np.float32) == pts[k, p])[0][0]) for k, a in enumerate(axes)]
        c = float(values[p])
        for k in range(len(axes)):
            if k not in keep:
                c *= weights[k][idx[k]]
        out[tuple(idx[k] for k in keep)] += c
    return out


def test_marginal_ref_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    lens = G.LENS5
    axes = [np.sort(rng.normal(size=L)).astype(np.float32) + 10 * k for k, L in enumerate(lens)]
    weights = [rng.normal(size=L) for L in lens]                         # mixed sign
    weights[3][1] = 0.0
    P = int(np.prod(lens))
    v = rng.uniform(0.1, 2.0, size=P)
    for keep in M.all_requests(len(lens)):
        got = M.marginal(v, lens, weights, keep)
        want = _brute(v, axes, weights, keep)
        assert got.shape == want.shape == M.table_shape(lens, keep)
        scale = np.abs(want).max() + 1.0
        assert np.max(np.abs(got - want)) <= 1e-13 * scale, keep
        # the scattered form (a window) agrees with the reshaped one, and windows add up
        parts = sum(M.marginal(v[a:b], lens, weights, keep, first=a) for a, b in ((0, 100), (100, 163), (163, P)))
        assert np.max(np.abs(parts - want)) <= 1e-13 * scale, keep
    lp = np.log(v).astype(np.float32)
    tabs = M.marginals_of_logpdf(lp, lens, weights, [(), (2, 4)])
    assert np.allclose(tabs[(2, 4)], M.marginal(np.exp(lp.astype(np.float64)), lens, weights, (2, 4)), rtol=0, atol=0)
    assert M.terms_per_bin(lens, (2, 4)) == 6 and M.terms_per_bin(lens, ()) == P
