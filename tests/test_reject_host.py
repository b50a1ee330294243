"""Truncated sampling on the CPU: df_flow_sample_region is declared, bound and exported; its
argument checks answer without a device; Region / Box / HalfSpaces validate in Python before
the library is touched; and the numpy restatement of the contract that the GPU tests compare
against (tests/reject_ref.py) is pinned on literals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
import reject_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
NAN = np.nan


def test_header_declares_and_signatures_bind_the_call():
    src = open(os.path.join(ROOT, "include", "densityflows_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+df_flow_sample_region\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "include/densityflows_hip.h does not declare df_flow_sample_region"
    assert len(m.group(1).split(",")) == 12
    res, args = _lib.SIGNATURES["df_flow_sample_region"]
    assert res is C.c_int and len(args) == 12
    assert hasattr(_lib.load(), "df_flow_sample_region")
    assert _lib.ABI_VERSION == 5 and "#define DF_ABI_VERSION 5" in src
    assert _lib.load().df_get_abi_version() == 5
    assert "#define DF_REGION_MAX_HALFSPACES 8" in src and _lib.DF_REGION_MAX_HALFSPACES == 8
    # the struct mirrors the header's: two int32 and four pointers
    assert C.sizeof(_lib.df_region) == 8 + 4 * C.sizeof(C.c_void_p)


def _region(d=2, n_half=0, lo=None, hi=None, a=None, b=None):
    keep = [np.ascontiguousarray(v, np.float32) if v is not None else None for v in (lo, hi, a, b)]
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float)) if v is not None else C.POINTER(C.c_float)()
    return _lib.df_region(d, n_half, *[fp(v) for v in keep]), keep


def _call(reg, chain=None, n_want=4, max_tries=400, round=0):
    lib = _lib.load()
    tried, acc = C.c_int64(-7), C.c_int64(-7)
    rc = lib.df_flow_sample_region(chain, None, None, n_want, C.byref(reg) if reg is not None else None, max_tries,
                                   round, 1, 0, C.byref(tried), C.byref(acc), None)
    return rc, lib.df_last_error().decode(), tried.value, acc.value


def test_bad_arguments_are_rejected_without_a_device():
    ok, ok_arrays = _region(lo=[0, 0], hi=[1, 1])      # (the arrays a df_region points to stay alive)
    rc, msg, tried, acc = _call(ok)
    assert rc == _lib.DF_ERR_INVALID and "null chain" in msg and (tried, acc) == (-7, -7)
    assert _call(None)[0] == _lib.DF_ERR_INVALID
    for n_half in (-1, 9):
        reg, keep = _region(n_half=n_half, a=np.zeros(18), b=np.zeros(9))
        rc, msg, _, _ = _call(reg)
        assert rc == _lib.DF_ERR_UNSUPPORTED and "half-spaces" in msg
    for kw in (dict(lo=[0, NAN], hi=[1, 1]), dict(lo=[0, 0], hi=[NAN, 1]),
               dict(n_half=1, a=[1, NAN], b=[0]), dict(n_half=1, a=[1, 1], b=[NAN])):
        reg, keep = _region(**kw)
        rc, msg, _, _ = _call(reg)
        assert rc == _lib.DF_ERR_INVALID and "NaN" in msg, kw
    reg, keep = _region(n_half=1)                       # half-spaces announced, arrays missing
    assert _call(reg)[0] == _lib.DF_ERR_INVALID
    assert _call(ok, n_want=-1)[0] == _lib.DF_ERR_SHAPE
    assert _call(ok, max_tries=-1)[0] == _lib.DF_ERR_SHAPE
    assert _call(ok, round=-4)[0] == _lib.DF_ERR_SHAPE
    assert _call(ok, round=(1 << 24) + 4)[0] == _lib.DF_ERR_UNSUPPORTED
    for d in (0, 65):
        reg, keep = _region(d=d)
        assert _call(reg)[0] == _lib.DF_ERR_SHAPE
    # an empty box and infinite bounds are legal: the call gets as far as the chain
    reg, keep = _region(lo=[1, -INF], hi=[0, INF])
    rc, msg, _, _ = _call(reg)
    assert rc == _lib.DF_ERR_INVALID and "null chain" in msg


def test_exports():
    for name in ("sample_with_rejection", "Box", "HalfSpaces", "Region"):
        assert getattr(dfa, name) is getattr(flows, name)
        assert name in flows.__all__


def test_region_validation_raises_before_the_library_loads(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(dfa.ArgumentError):
        dfa.Box([0, NAN], 1)
    with pytest.raises(dfa.ArgumentError):
        dfa.Box(0, NAN)
    with pytest.raises(dfa.DimensionMismatch):
        dfa.Box([0, 0], [1, 1, 1])
    with pytest.raises(dfa.DimensionMismatch):
        dfa.Box(np.zeros((2, 2)), 1)
    with pytest.raises(dfa.ArgumentError):
        dfa.HalfSpaces([[1, NAN]], [0])
    with pytest.raises(dfa.ArgumentError):
        dfa.HalfSpaces([[1, 1]], [NAN])
    with pytest.raises(dfa.DimensionMismatch):
        dfa.HalfSpaces([[1, 1], [2, 2]], [0])
    with pytest.raises(dfa.DimensionMismatch):
        dfa.HalfSpaces([1, 1], [0, 1])
    with pytest.raises(dfa.UnsupportedError):
        dfa.HalfSpaces(np.ones((9, 2)), np.zeros(9))
    with pytest.raises(dfa.ArgumentError):
        dfa.Region(box=([0, 0], [1, 1]))
    with pytest.raises(dfa.ArgumentError):
        dfa.Region(halfspaces=dfa.Box())
    # a region against the flow's d
    with pytest.raises(dfa.DimensionMismatch):
        dfa.Region(dfa.Box([0, 0], 1)).arrays(3)
    with pytest.raises(dfa.DimensionMismatch):
        dfa.Region(None, dfa.HalfSpaces([1, 1], 0)).arrays(3)
    # scalars broadcast to d; an empty box and infinities are legal; no box is the infinite one
    lo, hi, A, b = dfa.Region(dfa.Box(-INF, [1, 2, 3]), dfa.HalfSpaces([1, 2, 3], 4)).arrays(3)
    assert lo.dtype == hi.dtype == A.dtype == b.dtype == np.float32
    assert lo.tolist() == [-INF] * 3 and hi.tolist() == [1, 2, 3] and A.tolist() == [[1, 2, 3]] and b.tolist() == [4]
    lo, hi, A, b = dfa.Region().arrays(2)
    assert lo.tolist() == [-INF, -INF] and hi.tolist() == [INF, INF] and A.shape == (0, 2) and b.shape == (0,)
    assert dfa.Box(1, 0).arrays(2)[0].tolist() == [1, 1]


def test_sample_with_rejection_checks_arguments_before_the_library(monkeypatch):
    from densityflows_amd.data import MetaData

    def no_load(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    rng = np.random.default_rng(0)
    ch = dfa.FlowChain(dfa.CouplingLayer(3, [1], n=1, rng=rng))
    flow = dfa.Flow(ch, metadata=MetaData("", 3, 1, np.zeros(1, np.float32), np.ones(1, np.float32)))
    box = dfa.Box(0, 1)
    with pytest.raises(dfa.ArgumentError):              # θ as an array: the reference has no such method
        dfa.sample_with_rejection(box, flow, 4, np.zeros((1, 4), np.float32))
    with pytest.raises(dfa.DimensionMismatch):
        dfa.sample_with_rejection(box, flow, 4, (0.5, 0.5))
    with pytest.raises(dfa.DimensionMismatch):
        dfa.sample_with_rejection(dfa.Box([0, 0], 1), flow, 4, (0.5,))
    with pytest.raises(dfa.ArgumentError):
        dfa.sample_with_rejection("x > 0", flow, 4, (0.5,))
    with pytest.raises(dfa.DimensionMismatch):
        dfa.sample_with_rejection(box, flow, 4, (0.5,), m=-1)


def test_predicate_on_literals():
    # six points of a 2-D region: box [0, 2] × [-1, 1] and x0 + 2·x1 <= 2.5
    x = np.array([[1.0, 0.5],      # inside
                  [2.0, 0.25],     # x0 exactly on hi, sum exactly on b: accepted
                  [2.0, 0.5],      # in the box, sum 3 > 2.5
                  [-0.1, 0.0],     # below lo
                  [NAN, 0.0],      # NaN rejects
                  [0.0, -1.0]],    # x1 exactly on lo
                 np.float32).T
    got = R.predicate(x, [0, -1], [2, 1], [[1, 2]], [2.5])
    assert got.dtype == bool and got.tolist() == [True, True, False, False, False, True]
    assert R.predicate(x, [0, -1], [2, 1]).tolist() == [True, True, True, False, False, True]
    assert R.predicate(x, A=[[1, 2]], b=[2.5]).tolist() == [True, True, False, True, False, True]
    assert R.predicate(x, -INF, INF).tolist() == [True, True, True, True, False, True]
    assert R.predicate(x).all()
    assert not R.predicate(x, 1, 0).any()               # an empty box


def test_predicate_rounds_every_operation_to_float32():
    # 2^24 + 1 is not a Float32: acc = 2^24, then + 1 stays 2^24 in Float32 (2^24 + 1 in fp64)
    x = np.array([[1.0, 1.0]], np.float32).T
    assert R.predicate(x, A=[[16777216.0, 1.0]], b=[16777216.0]).tolist() == [True]
    # left to right: (1e8 + 1) - 1e8 = 0 in Float32, whereas 1e8 - 1e8 + 1 = 1
    x3 = np.array([[1.0, 1.0, 1.0]], np.float32).T
    assert R.predicate(x3, A=[[1e8, 1.0, -1e8]], b=[0.5]).tolist() == [True]
    assert R.predicate(x3, A=[[1e8, -1e8, 1.0]], b=[0.5]).tolist() == [False]
    # each product is rounded before it is added: v² = 1 + 2^-11 + 2^-24 rounds to w = 1 + 2^-11,
    # so -w + v·v is exactly 0, where a fused multiply-add would leave 2^-24
    v, w = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -11)
    xv = np.array([[1.0, v]], np.float32).T
    assert R.predicate(xv, A=[[-w, v]], b=[0.0]).tolist() == [True]
    assert R.predicate(xv, A=[[w, -v]], b=[-1e-9]).tolist() == [False]


def test_first_accepted_on_literals():
    cands = np.arange(20, dtype=np.float32).reshape(10, 2).T          # candidate k = (2k, 2k + 1)
    mask = np.array([0, 1, 1, 0, 0, 1, 0, 1, 1, 0], bool)
    rows, tried, acc = R.first_accepted(cands, mask, 3, 100)          # the third acceptance: index 5
    assert rows.T.tolist() == [[2, 3], [4, 5], [10, 11]] and (tried, acc) == (6, 3)
    rows, tried, acc = R.first_accepted(cands, mask, 5, 100)          # the last one fills it
    assert rows[0].tolist() == [2, 4, 10, 14, 16] and (tried, acc) == (9, 5)
    rows, tried, acc = R.first_accepted(cands, mask, 6, 100)          # runs out: all examined
    assert rows.shape == (2, 5) and (tried, acc) == (10, 5)
    rows, tried, acc = R.first_accepted(cands, mask, 3, 5)            # max_tries cuts before index 5
    assert rows.T.tolist() == [[2, 3], [4, 5]] and (tried, acc) == (5, 2)
    rows, tried, acc = R.first_accepted(cands, mask, 3, 6)            # index 5 is the last examined
    assert (tried, acc) == (6, 3)
    rows, tried, acc = R.first_accepted(cands, np.zeros(10, bool), 1, 7)
    assert rows.shape == (2, 0) and (tried, acc) == (7, 0)


def test_adaptive_schedule_is_multiples_of_four_within_its_clamps():
    for n in (1, 63, 1000, 1 << 20, 1 << 40):
        r = flows._first_round(n)
        assert r % 4 == 0 and 1 << 10 <= r <= 1 << 22
    assert flows._first_round(1000) == 2000 and flows._first_round(1 << 20) == 1 << 21
    assert flows._next_round(100, 2000, 900, 2000) == 1024             # clamped from below
    assert flows._next_round(10, 2000, 0, 2000) == 4000                # nothing accepted yet: double
    assert flows._next_round(1 << 20, 1 << 21, 1000, 1 << 21) == 1 << 22
    # remaining / rate · 5/4 + 64, rounded up to a multiple of 4
    assert flows._next_round(5000, 10000, 5001, 10000) == (-(-(5000 * 10000 * 5) // (5001 * 4)) + 64 + 3) // 4 * 4
