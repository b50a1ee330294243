"""Host side of sampling with densities and the moment reductions (df_moments.hip), on CPU:
the four calls are declared, bound and exported at ABI 5; their argument errors come back
before any device work; ScoreMoments' arithmetic is numpy's; the Python wrappers refuse bad
arguments before the library is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib
from densityflows_amd.data import MetaData
from helpers import spec_to_element
from train_edge_cases import SPECS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"df_flow_sample_logpdf": 9, "df_flow_sample_logpdf_moments": 8, "df_train_score_moments": 7,
         "df_train_fisher": 8}


def _header():
    src = open(os.path.join(ROOT, "include", "densityflows_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_calls_declared_bound_and_exported():
    src = _header()
    lib = _lib.load()
    for name, arity in CALLS.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == arity, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity, name
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", src)
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION


def test_argument_errors_before_device_work():
    """No device exists here: every status below is returned by a check that stands before
    the first use of the handle (a non-null handle is a buffer that is never read)."""
    lib = _lib.load()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    null = C.c_void_p(0)
    out = C.c_void_p(C.addressof(C.create_string_buffer(8 * 16)))
    u = C.c_uint64
    # a null chain or trainer
    assert lib.df_flow_sample_logpdf(null, out, out, null, 0, 4, u(1), u(0), null) == _lib.DF_ERR_INVALID
    assert lib.df_flow_sample_logpdf_moments(null, null, 4, 0, u(1), u(0), out, null) == _lib.DF_ERR_INVALID
    assert lib.df_train_score_moments(null, out, null, 4, out, 0, null) == _lib.DF_ERR_INVALID
    assert lib.df_train_fisher(null, null, 4, 0, u(1), u(0), out, null) == _lib.DF_ERR_INVALID
    # a negative batch, n_samples or chunk
    assert lib.df_flow_sample_logpdf(fake, out, out, null, 0, -1, u(1), u(0), null) == _lib.DF_ERR_SHAPE
    assert lib.df_flow_sample_logpdf_moments(fake, null, -1, 0, u(1), u(0), out, null) == _lib.DF_ERR_SHAPE
    assert lib.df_flow_sample_logpdf_moments(fake, null, 4, -1, u(1), u(0), out, null) == _lib.DF_ERR_SHAPE
    assert lib.df_train_score_moments(fake, out, null, -1, out, 0, null) == _lib.DF_ERR_SHAPE
    assert lib.df_train_fisher(fake, null, -1, 0, u(1), u(0), out, null) == _lib.DF_ERR_SHAPE
    assert lib.df_train_fisher(fake, null, 4, -1, u(1), u(0), out, null) == _lib.DF_ERR_SHAPE
    # a chunk above 2^24
    big = (1 << 24) + 1
    assert lib.df_flow_sample_logpdf_moments(fake, null, 4, big, u(1), u(0), out, null) == _lib.DF_ERR_UNSUPPORTED
    assert lib.df_train_fisher(fake, null, 4, big, u(1), u(0), out, null) == _lib.DF_ERR_UNSUPPORTED
    assert b"2^24" in lib.df_last_error()
    with pytest.raises(_lib.UnsupportedError):
        _lib.check(lib.df_train_fisher(fake, null, 4, big, u(1), u(0), out, null))


def test_score_moments_arithmetic():
    rng = np.random.default_rng(3)
    n, N = 3, 50
    lp = rng.standard_normal(N) * 2 - 5
    g = rng.standard_normal((n, N))
    block = np.concatenate([[N, lp.sum(), (lp * lp).sum()], g.sum(axis=1), (g @ g.T).ravel(order="F")])
    m = dfa.ScoreMoments(block, n)
    assert m.count == N and m.n == n
    np.testing.assert_array_equal(m.score_sum, g.sum(axis=1))
    np.testing.assert_array_equal(m.outer, g @ g.T)
    np.testing.assert_array_equal(m.fisher, (g @ g.T) / N)
    np.testing.assert_array_equal(m.mean_score, g.sum(axis=1) / N)
    np.testing.assert_array_equal(m.score_cov, (g @ g.T) / N - np.outer(g.sum(axis=1) / N, g.sum(axis=1) / N))
    np.testing.assert_allclose(m.score_cov, np.cov(g, bias=True), rtol=1e-12, atol=1e-14)
    assert m.entropy == -lp.sum() / N
    mean = lp.sum() / N
    assert m.entropy_stderr == np.sqrt(((lp * lp).sum() / N - mean * mean) / N)
    np.testing.assert_allclose(m.entropy_stderr, lp.std() / np.sqrt(N), rtol=1e-10)
    # column-major: entry (a, b) of the block is outer[a, b]
    asym = np.arange(3 + 2 + 4, dtype=np.float64)
    assert dfa.ScoreMoments(asym, 2).outer[1, 0] == 6.0 and dfa.ScoreMoments(asym, 2).outer[0, 1] == 7.0
    # n = 0: three entries, a 0 × 0 matrix
    m0 = dfa.ScoreMoments([4.0, -8.0, 16.5], 0)
    assert m0.fisher.shape == (0, 0) and m0.mean_score.shape == (0,) and m0.entropy == 2.0
    with pytest.raises(_lib.DimensionMismatch):
        dfa.ScoreMoments(np.zeros(4), 1)


def test_entropy_stderr_guard():
    """Rounding can leave E[lp²] − E[lp]² a hair below zero for (nearly) constant lp: the
    variance is clamped at 0 instead of giving a NaN."""
    lp = np.full(7, 0.1)
    s, q = lp.sum(), (lp * lp).sum()
    var = q / 7 - (s / 7) * (s / 7)
    m = dfa.ScoreMoments([7.0, s, q], 0)
    assert m.entropy_stderr == np.sqrt(max(0.0, var) / 7) and np.isfinite(m.entropy_stderr)
    # a block whose raw variance is negative for certain
    m = dfa.ScoreMoments([4.0, 8.0, 16.0 - 1e-9], 0)
    assert 16.0 - 1e-9 < 16.0 and m.entropy_stderr == 0.0


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
    for call in (lambda **k: dfa.fisher_information(flow, k.pop("theta", (1.25,)), k.pop("n_samples", 16), **k),
                 lambda **k: dfa.entropy(flow, k.pop("n_samples", 16), k.pop("theta", (1.25,)), **k)):
        with pytest.raises(_lib.DimensionMismatch, match="tuple"):
            call(theta=(1.0, 2.0))
        with pytest.raises(_lib.DimensionMismatch, match="tuple"):
            call(theta=())
        with pytest.raises(_lib.DimensionMismatch, match="tuple"):
            call(theta=np.array([1.25], np.float32))
        with pytest.raises(_lib.DimensionMismatch, match="n_samples"):
            call(n_samples=-1)
        with pytest.raises(_lib.UnsupportedError, match="2\\^24"):
            call(chunk=(1 << 24) + 1)
        with pytest.raises(_lib.DimensionMismatch, match="chunk"):
            call(chunk=-4)
    with pytest.raises(AssertionError, match="dimensions θ"):
        dfa.sample_logpdf(flow, (3,), (1.0, 2.0), seed=1)
    with pytest.raises(AssertionError, match="dimensions θ"):
        dfa.sample_logpdf(flow, (3,), None, seed=1)
    with pytest.raises(AssertionError, match="dimensions θ"):
        dfa.sample_logpdf(flow, (3,), np.zeros((1, 4), np.float32), seed=1)
