"""Host side of the resampling call (df_resample.hip), on CPU: df_draw_resample is declared, bound
and exported at ABI 5; its argument errors come back before any device work, in the stated order,
each with a message naming the rule; the Python wrappers refuse bad arguments before the library
is touched; the pure-integer reference of tests/resample_ref.py reproduces the Random123
known-answer vectors of Philox4x32-10 and the identities its picks must satisfy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib, flows
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calls_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "densityflows_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    m = re.search(r"^int\s+df_draw_resample\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, "df_draw_resample is not declared in the header"
    assert len(m.group(1).split(",")) == 13
    res, args = _lib.SIGNATURES["df_draw_resample"]
    assert res is C.c_int and len(args) == 13
    assert hasattr(lib, "df_draw_resample"), "df_draw_resample is not exported"
    for name, value in (("DF_RESAMPLE_SYSTEMATIC", 0), ("DF_RESAMPLE_STRATIFIED", 1), ("DF_RESAMPLE_MULTINOMIAL", 2),
                        ("DF_RESAMPLE_LDS_DRAWS", 4096)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", src), name
    assert re.search(r"#define\s+DF_ABI_VERSION\s+5\b", src)
    assert lib.df_get_abi_version() == 5 == _lib.ABI_VERSION
    assert "run_draw_resample" in dfa.hip.__all__ and hasattr(dfa.hip, "run_draw_resample")
    for name in ("resample_indices", "resample", "importance_resample"):
        assert name in flows.__all__ and hasattr(dfa, name)
    assert flows.RESAMPLE_METHODS == R.METHODS and flows.RESAMPLE_LDS_DRAWS == 4096


def _message():
    return _lib.load().df_last_error().decode("utf-8")


def _fake(n_bytes=256):
    """A non-null, 16-byte aligned pointer that is never read, the same 4 and 8 bytes on."""
    buf = C.create_string_buffer(n_bytes + 16)
    at = (C.addressof(buf) + 15) & ~15
    return buf, C.c_void_p(at), C.c_void_p(at + 4), C.c_void_p(at + 8)


def test_argument_errors_before_device_work():
    """No device exists here: every status below is returned by a check that stands before the
    first launch."""
    lib = _lib.load()
    keep, ok, off4, off8 = _fake()
    null = C.c_void_p(0)
    big = (1 << 24) + 4

    def call(xs=ok, w=ok, ws=null, d=5, n_points=4, n_draws=8, n_out=8, method=0, out=ok, idx=ok):
        return lib.df_draw_resample(xs, w, ws, d, n_points, n_draws, n_out, method, 7, 0, out, idx, null)

    # every rule, its status and a word of its message
    for bad in (-1, 3, 99):
        assert call(method=bad) == _lib.DF_ERR_INVALID and "method" in _message(), bad
    assert call(n_points=-1) == _lib.DF_ERR_SHAPE and "point count" in _message()
    for bad in (0, -4, 6, 1023):
        assert call(n_draws=bad) == _lib.DF_ERR_INVALID and "n_draws" in _message() and "multiple of 4" in _message(), bad
    assert call(n_draws=big, ws=ok) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message() and "n_draws" in _message()
    for bad in (0, -4, 6, 1023):
        assert call(n_out=bad) == _lib.DF_ERR_INVALID and "n_out" in _message() and "multiple of 4" in _message(), bad
    assert call(n_out=big) == _lib.DF_ERR_UNSUPPORTED and "2^24" in _message() and "n_out" in _message()
    assert call(w=null) == _lib.DF_ERR_INVALID and "null w" in _message()
    assert call(w=off4) == _lib.DF_ERR_INVALID and "w must be 16-byte aligned" in _message()
    assert call(w=off8) == _lib.DF_ERR_INVALID and "16-byte aligned" in _message()
    assert call(out=null, idx=null) == _lib.DF_ERR_INVALID and "no output" in _message()
    for bad in (0, -1, 65):
        assert call(d=bad) == _lib.DF_ERR_INVALID and "1 .. 64" in _message(), bad
    assert call(xs=null) == _lib.DF_ERR_INVALID and "null xs" in _message()
    assert call(xs=off4) == _lib.DF_ERR_INVALID and "xs must be 16-byte aligned" in _message()
    assert call(n_draws=4100) == _lib.DF_ERR_INVALID and "cdf_ws" in _message()
    assert call(n_draws=4100, ws=off4) == _lib.DF_ERR_INVALID and "cdf_ws" in _message()
    assert call(n_points=1 << 61) == _lib.DF_ERR_SHAPE and "int64" in _message()
    assert call(n_points=1 << 40, n_draws=1 << 20, ws=ok) == _lib.DF_ERR_SHAPE
    assert call(n_points=1 << 40, n_out=1 << 20) == _lib.DF_ERR_SHAPE
    # picks only: xs and d are not looked at
    assert call(n_points=0, xs=null, d=0, out=null) == _lib.DF_OK
    assert call(n_points=0, xs=off4, d=99, out=null) == _lib.DF_OK
    # cdf_ws is not demanded at n_draws = 4096, demanded at 4100; 8-byte alignment is enough
    assert call(n_points=0, n_draws=4096) == _lib.DF_OK
    assert call(n_points=0, n_draws=4096, ws=off4) == _lib.DF_OK          # ignored
    assert call(n_points=0, n_draws=4100) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=4100, ws=off8) == _lib.DF_OK
    # the order: method, the point count, n_draws, n_out, w, the outputs, d, xs, cdf_ws, the size
    assert call(method=3, n_points=-1) == _lib.DF_ERR_INVALID and "method" in _message()
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, n_out=6) == _lib.DF_ERR_INVALID and "n_draws" in _message()
    assert call(n_draws=big, n_out=6) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_out=6, w=null) == _lib.DF_ERR_INVALID and "n_out" in _message()
    assert call(n_out=big, w=null) == _lib.DF_ERR_UNSUPPORTED
    assert call(w=null, out=null, idx=null) == _lib.DF_ERR_INVALID and "null w" in _message()
    assert call(w=off4, out=null, idx=null) == _lib.DF_ERR_INVALID and "aligned" in _message()
    assert call(out=null, idx=null, d=0) == _lib.DF_ERR_INVALID and "no output" in _message()
    assert call(d=0, xs=null) == _lib.DF_ERR_INVALID and "1 .. 64" in _message()
    assert call(xs=null, n_draws=4100) == _lib.DF_ERR_INVALID and "null xs" in _message()
    assert call(xs=off4, n_draws=4100) == _lib.DF_ERR_INVALID and "xs must be" in _message()
    assert call(n_draws=4100, n_points=1 << 61) == _lib.DF_ERR_INVALID and "cdf_ws" in _message()
    # the same rules hold for an empty call
    assert call(n_points=0, method=3) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_draws=big, ws=ok) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, n_out=6) == _lib.DF_ERR_INVALID
    assert call(n_points=0, n_out=big) == _lib.DF_ERR_UNSUPPORTED
    assert call(n_points=0, w=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, w=off4) == _lib.DF_ERR_INVALID
    assert call(n_points=0, out=null, idx=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, d=65) == _lib.DF_ERR_INVALID
    assert call(n_points=0, xs=null) == _lib.DF_ERR_INVALID
    assert call(n_points=0, xs=off4) == _lib.DF_ERR_INVALID
    # a sound empty call launches nothing
    for method in (0, 1, 2):
        assert call(n_points=0, method=method) == _lib.DF_OK
        assert call(n_points=0, method=method, out=null) == _lib.DF_OK
        assert call(n_points=0, method=method, idx=null) == _lib.DF_OK
    with pytest.raises(_lib.ArgumentError, match="n_out"):
        _lib.check(call(n_out=6))
    with pytest.raises(_lib.UnsupportedError):
        _lib.check(call(n_out=big))
    with pytest.raises(_lib.DimensionMismatch):
        _lib.check(call(n_points=-1))
    del keep


def test_python_argument_errors(monkeypatch):
    """Raised before the library is touched: the runner and Flow.hip are never called."""
    def touched(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(dfa.hip, "run_draw_resample", touched)
    monkeypatch.setattr(dfa.hip, "run_importance_weights", touched)
    monkeypatch.setattr(dfa.Flow, "hip", touched)
    w = np.ones((3, 8), np.float32)
    q = np.zeros((3, 8, 5), np.float32)
    calls = (lambda **k: dfa.resample_indices(k.pop("weights", w), seed=1, **k),
             lambda **k: dfa.resample(k.pop("draws", q), k.pop("weights", w), seed=1, **k))
    for fn in calls:
        for bad in ("residual", "Systematic", 0, None):
            with pytest.raises(_lib.ArgumentError, match="unknown resampling method"):
                fn(method=bad)
        with pytest.raises(_lib.ArgumentError, match="weights must be Float32"):
            fn(weights=w.astype(np.float64))
        for bad in (np.ones(8, np.float32), np.ones((3, 8, 1), np.float32)):
            with pytest.raises(_lib.DimensionMismatch, match="weights"):
                fn(weights=bad)
        for bad in (6, 0, -4, 1023):
            with pytest.raises(_lib.ArgumentError, match="n_out must be a positive multiple of 4"):
                fn(n_out=bad)
        with pytest.raises(_lib.UnsupportedError, match="n_out"):
            fn(n_out=(1 << 24) + 4)
    with pytest.raises(_lib.ArgumentError, match="multiple of 4"):
        dfa.resample_indices(np.ones((3, 6), np.float32), seed=1)
    with pytest.raises(_lib.ArgumentError, match="draws must be Float32"):
        dfa.resample(q.astype(np.float64), w, seed=1)
    with pytest.raises(_lib.DimensionMismatch, match=r"\(M, N, d\)"):
        dfa.resample(q[0], w, seed=1)
    with pytest.raises(_lib.ArgumentError, match="1 .. 64"):
        dfa.resample(np.zeros((3, 8, 65), np.float32), w, seed=1)
    for bad in (np.ones((3, 12), np.float32), np.ones((4, 8), np.float32)):
        with pytest.raises(_lib.DimensionMismatch, match=r"weights must have size \(3, 8\)"):
            dfa.resample(q, bad, seed=1)
    iw = dfa.ImportanceWeights(np.ones((2, 8), np.float32), np.tile([0.0, 8.0, 8.0, 8.0], (2, 1)), 8)
    with pytest.raises(_lib.DimensionMismatch, match=r"weights must have size \(3, 8\)"):
        dfa.resample(q, iw, seed=1)
    # importance_resample: method and n_out before the flow is touched
    target = lambda draws, theta: touched()
    th = np.ones((1, 3, 2), np.float32)
    with pytest.raises(_lib.ArgumentError, match="unknown resampling method"):
        dfa.importance_resample(object(), th, target, method="residual", seed=1)


# ---------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------

def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32-10."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, out in kat:
        assert tuple(int(v) for v in R.philox4x32_10(np.array(ctr, np.uint64), key)) == out
    # a batch of counters is the counters one by one
    both = R.philox4x32_10(np.array([kat[0][0], kat[2][0]], np.uint64), kat[2][1])
    assert tuple(int(v) for v in both[1]) == kat[2][2]


def test_quantise():
    assert R.quantise([1.0]) == [1 << 31]
    assert R.quantise([0.75, 0.5]) == [3 << 30, 1 << 31]
    for top in (1.0, 3.5e-42, 2.0 ** 127, 1e-3):                      # any scale, a subnormal one included
        top = float(np.float32(top))
        q = R.quantise([top, top / 2, top / 4])
        assert (1 << 31) <= q[0] <= (1 << 32) and q[1] in (q[0] // 2, q[0] // 2 + 1), top
    # below 2^−33 of the scale 2^e (here e = 1), NaN, ±inf, negative, ±0: q = 0
    tiny = [2.0 ** -33, 2.0 ** -40, 1e-30, np.nan, np.inf, -np.inf, -1.0, -1e-30, 0.0, -0.0]
    q = R.quantise([1.0] + tiny)
    assert q[0] == 1 << 31 and q[1:] == [0] * len(tiny)
    assert R.quantise([1.0, 1.5 * 2.0 ** -31]) == [1 << 31, 2]       # 1.5 rounds to even: 2
    assert R.quantise([1.0, 2.5 * 2.0 ** -31]) == [1 << 31, 2]       # 2.5 rounds to even: 2
    assert R.quantise([1.0, 2.0 ** -31]) == [1 << 31, 1]
    assert R.quantise([1.0, 2.0 ** -32]) == [1 << 31, 0]             # 2^−33 of the scale: 0.5 rounds to even: 0
    assert R.quantise([1.0, 1.25 * 2.0 ** -32]) == [1 << 31, 1]
    # +inf does not set the scale
    assert R.quantise([np.inf, 0.5, np.nan]) == [0, 1 << 31, 0]
    # no weight takes part
    assert R.quantise([np.nan, -1.0, 0.0, np.inf]) == [0, 0, 0, 0]


@pytest.mark.parametrize("N", [4, 12, 260])
def test_unit_weights_systematic_identity(N):
    w = np.ones((3, N), np.float32)
    for K in (N, 2 * N):
        for seed in (0, 1, 2 ** 63 + 5):
            idx = R.picks(w, K, "systematic", seed, 11)
            np.testing.assert_array_equal(idx, np.tile(np.arange(K) * N // K, (3, 1)))


def _weights(M, N, seed):
    rng = np.random.default_rng(seed)
    w = np.exp(rng.uniform(-30.0, 0.0, (M, N))).astype(np.float32)
    w[:, 1] = 0.0
    w[:, 2] = np.nan
    return w


@pytest.mark.parametrize("N", [4, 12, 260])
@pytest.mark.parametrize("method", ["systematic", "stratified", "multinomial"])
def test_picks_against_brute_force(N, method):
    """The search agrees with a scan over j of the cross-multiplied comparison; excluded draws are
    never picked; the systematic multiplicity of draw j lies within floor / ceil of K·q_j/T."""
    M, seed, offset = 3, 0x1234567887654321, 5
    w = _weights(M, N, N)
    for K in (4, N, 1028):
        idx = R.picks(w, K, method, seed, offset)
        assert idx.shape == (M, K) and idx.dtype == np.int32
        num, D = R.numerators(M, K, R.METHODS[method], seed, offset)
        for i in range(M):
            q = R.quantise(w[i])
            c = R.scan(q)
            T = c[-1]
            assert q[1] == 0 and q[2] == 0 and max(q) >= 1 << 31 and T < 1 << 56
            for k in range(K):
                hits = [j for j in range(N) if c[j] * D <= num[i, k] * T < c[j + 1] * D]
                assert hits == [int(idx[i, k])], (i, k)
                assert q[hits[0]] > 0
            if method != "multinomial":
                assert np.all(np.diff(idx[i]) >= 0)
            if method == "systematic":
                count = np.bincount(idx[i], minlength=N)
                for j in range(N):
                    assert K * q[j] // T <= count[j] <= -((-K * q[j]) // T), (i, j)


def test_degenerate_point_and_gather():
    w = _weights(3, 12, 0)
    w[1] = [np.nan, -1.0, 0.0, np.inf] * 3
    draws = np.random.default_rng(1).standard_normal((3, 12, 5)).astype(np.float32)
    for method in R.METHODS:
        idx = R.picks(w, 8, method, 3)
        assert np.all(idx[1] == -1) and np.all(idx[[0, 2]] >= 0) and np.all(idx < 12)
        out = R.gather(draws, idx)
        assert out.shape == (3, 8, 5)
        assert np.all(out[1].view(np.uint32) == 0x7fc00000)
        for i in (0, 2):
            for k in range(8):
                np.testing.assert_array_equal(out[i, k].view(np.uint32), draws[i, idx[i, k]].view(np.uint32))
    # a call on the points [a, b) with the offset advanced reproduces the whole call's picks
    for method, per in (("systematic", 1), ("stratified", 8 // 4), ("multinomial", 8 // 2)):
        whole = R.picks(w, 8, method, 9, 100)
        np.testing.assert_array_equal(R.picks(w[2:], 8, method, 9, 100 + 2 * per), whole[2:])
