"""GPU tests of the weighted histogram call (df_whist.hip): df_draw_weighted_histograms and its
Python mirrors weighted_histograms / importance_posterior_histograms.

A bin is an integer sum of quantised weights: every comparison with the host reference
(tests/wquantile_ref.py: uint64 numpy on histogram_ref's bin rule) is ``==`` on bytes, and no
tolerance appears anywhere.  Every output buffer is pre-filled with a sentinel no sum can equal
(−1: all 64 bits set, above 2^56) and followed by GUARD words that must survive.

The kernel has df_draw_histograms' three mappings by N = n_draws: a wave per point up to 256, a
workgroup per point up to S = HIST_SPLIT_DRAWS, and above S a point's draws divided among
ceil(N / S) workgroups whose tables merge with 64-bit integer atomic adds.  A table past a quarter
of the tables' budget (above 2048 bins: 90 x 90) takes the workgroup mapping at every N.

No test states a statistical claim: the models are untrained.
"""
import ctypes as C

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib
import histogram_ref as H
import wquantile_ref as W
from test_gpu_wquantiles import FILL_SCALE, GUARD, _bits, _check_scale, _flow
from test_gpu_train import _inputs

pytestmark = pytest.mark.gpu

FILL = -1
S = dfa.HIST_SPLIT_DRAWS
SHAPES = [(1, 4), (3, 12), (17, 64), (5, 68), (3, 256), (3, 260), (257, 4), (2, 4100)]
DIMS = [1, 5, 8, 32, 61]


def _wh(cuda, x, w, edges, keep, flat=None):
    """One df_draw_weighted_histograms call on numpy draws (M, N, d) and weights (M, N) →
    (sums (M, T) uint64, scale (M, 2) int64).  ``flat``: the edges array as the device gets it."""
    import torch

    M, N, d = x.shape
    bins = H.bins_of(edges)
    T = sum(H.sizes(keep, bins))
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    wb = torch.from_numpy(np.ascontiguousarray(w)).to(cuda)
    eb = torch.from_numpy(H.flat_edges(edges) if flat is None else np.asarray(flat, np.float32)).to(cuda)
    out = torch.full((M * T + GUARD,), FILL, dtype=torch.int64, device=cuda)
    sc = torch.full((2 * M + GUARD,), FILL_SCALE, dtype=torch.int64, device=cuda)
    dfa.hip.run_draw_weighted_histograms(xs, wb, d, M, N, eb, bins, keep, out, sc)
    torch.cuda.synchronize()
    v, s = out.cpu().numpy(), sc.cpu().numpy()
    assert np.all(v[M * T:] == FILL), "sums_out written past n_points · T"
    assert np.all(v[:M * T] != FILL), "sums_out not fully written"
    assert np.all(s[2 * M:] == FILL_SCALE) and np.all(s[:2 * M] != FILL_SCALE)
    return v[:M * T].view(np.uint64).reshape(M, T).copy(), s[:2 * M].reshape(M, 2).copy()


def _edges8(d, bins=8):
    return [np.linspace(-2.0 - 0.03 * k, 2.0 + 0.05 * k, bins + 1).astype(np.float32) for k in range(d)]


def _draws(M, N, d, edges, seed):
    rng = np.random.default_rng(seed)
    return H.plant(rng.standard_normal((M, N, d)).astype(np.float32), edges, rng), rng


# ---------------------------------------------------------------------------
# 1. against the integer reference: the corner at 8 bins, every weight pattern
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_weighted_histograms_exact(cuda, d, M, N):
    edges = _edges8(d)
    keep = H.corner(H.bins_of(edges))
    x, rng = _draws(M, N, d, edges, 1000 * d + N + M)
    for name, w in W.weight_patterns(M, N, rng).items():
        got, s = _wh(cuda, x, w, edges, keep)
        _check_scale(s, w)
        np.testing.assert_array_equal(got, W.blocks(x, w, edges, keep), err_msg=name)
        if name == "hostile" and M > 1:                    # the empty point among others
            assert (s[M // 2] == 0).all() and not got[M // 2].any()


@pytest.mark.parametrize("M,N", [(3, 64), (2, 260), (2, 4100)])
def test_the_largest_table(cuda, M, N):
    """One 90 x 90 table, 8100 bins of 8 bytes: the largest that fits; a workgroup per point at every N."""
    d = 3
    edges = [np.linspace(-2.5, 2.5, 91).astype(np.float32), None, np.linspace(-2.0, 3.0, 91).astype(np.float32)]
    x, rng = _draws(M, N, d, edges, N)
    for name in ("lognormal3", "hostile"):
        w = W.weight_patterns(M, N, rng)[name]
        got, s = _wh(cuda, x, w, edges, [(0, 2)])
        _check_scale(s, w)
        np.testing.assert_array_equal(got, W.blocks(x, w, edges, [(0, 2)]), err_msg=name)


# ---------------------------------------------------------------------------
# 2. unit weights: df_draw_histograms' counts shifted left by 31, on the device
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,d", [(5, 68, 5), (3, 260, 8), (2, 4100, 5), (3, 256, 32)])
def test_unit_weights_are_shifted_counts(cuda, M, N, d):
    import torch

    edges = _edges8(d)
    keep = H.corner(H.bins_of(edges))
    bins = H.bins_of(edges)
    x, _ = _draws(M, N, d, edges, N + d)
    got, s = _wh(cuda, x, np.ones((M, N), np.float32), edges, keep)
    assert (s[:, 0] == 1).all() and (s[:, 1] == N << 31).all()
    counts = torch.empty((M, got.shape[1]), dtype=torch.int32, device=cuda)
    dfa.hip.run_draw_histograms(torch.from_numpy(x).to(cuda), d, M, N, torch.from_numpy(H.flat_edges(edges)).to(cuda),
                                bins, keep, counts)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, counts.cpu().numpy().astype(np.uint64) << np.uint64(31))


# ---------------------------------------------------------------------------
# 3. the split path: 64-bit global adds; the bytes do not depend on the split
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N", [S - 4, S, S + 4, 2 * S + 4])
@pytest.mark.parametrize("d", [5, 32])
def test_split_path(cuda, monkeypatch, d, N):
    M = 2
    edges = _edges8(d)
    keep = H.corner(H.bins_of(edges))
    x, rng = _draws(M, N, d, edges, N + d)
    w = W.weight_patterns(M, N, rng)["lognormal3"]
    monkeypatch.delenv("DF_HIST_SPLIT_DRAWS", raising=False)
    got, s = _wh(cuda, x, w, edges, keep)
    _check_scale(s, w)
    np.testing.assert_array_equal(got, W.blocks(x, w, edges, keep))
    monkeypatch.setenv("DF_HIST_SPLIT_DRAWS", "512")
    again, s2 = _wh(cuda, x, w, edges, keep)
    np.testing.assert_array_equal(again, got)
    np.testing.assert_array_equal(s2, s)


# ---------------------------------------------------------------------------
# 4. mass conservation; independence of the other points; two calls
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N", [68, 260, 4100])
def test_mass_conservation(cuda, N):
    """A 1-D table with the edges (−inf, +inf) sums to T minus the q of the NaN draws."""
    M, d = 3, 2
    rng = np.random.default_rng(N)
    x = rng.standard_normal((M, N, d)).astype(np.float32)
    x[:, ::7, 1] = np.nan
    x[:, 1::7, 1] = np.inf
    x[:, 2::7, 1] = -np.inf
    edges = [None, np.array([-np.inf, np.inf], np.float32)]
    for name, w in W.weight_patterns(M, N, rng).items():
        got, s = _wh(cuda, x, w, edges, [(1,)])
        _, T, q = W.scales(w)
        nan_q = (q * np.isnan(x[:, :, 1])).sum(axis=1, dtype=np.uint64)
        np.testing.assert_array_equal(got[:, 0], T.astype(np.uint64) - nan_q, err_msg=name)
        np.testing.assert_array_equal(s[:, 1], T)


@pytest.mark.parametrize("N", [12, 260])
def test_independent_of_the_other_points(cuda, N):
    M, d = 257, 5
    edges = _edges8(d)
    keep = H.corner(H.bins_of(edges))
    x, rng = _draws(M, N, d, edges, N)
    w = W.weight_patterns(M, N, rng)["lognormal3"]
    all_, s = _wh(cuda, x, w, edges, keep)
    again, s2 = _wh(cuda, x, w, edges, keep)
    np.testing.assert_array_equal(all_, again)
    np.testing.assert_array_equal(s, s2)
    for i in (0, 130, 256):
        one, s1 = _wh(cuda, x[i:i + 1], w[i:i + 1], edges, keep)
        np.testing.assert_array_equal(one[0], all_[i])
        np.testing.assert_array_equal(s1[0], s[i])


# ---------------------------------------------------------------------------
# 5. hostile edges stay in bounds
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["unsorted", "all equal", "nan"])
def test_hostile_edges_stay_in_bounds(cuda, kind):
    """The C call does not read the edges; its search is bounded by construction, so that for any
    edge content every add lands in the point's own block or is dropped.  Checked on memory the
    call owns: the guards survive, every word is written, every sum is at most T."""
    M, N, d = 3, 68, 5
    rng = np.random.default_rng(17)
    edges = _edges8(d)
    x = H.plant(rng.standard_normal((M, N, d)).astype(np.float32), edges, rng)
    flat = H.flat_edges(edges)
    if kind == "unsorted":
        flat = rng.permutation(flat)
    elif kind == "all equal":
        flat = np.full_like(flat, 0.25)
    else:
        flat = flat.copy()
        flat[rng.permutation(flat.size)[:flat.size // 2]] = np.nan
        flat[-1] = np.nan
    w = W.weight_patterns(M, N, rng)["lognormal3"]
    got, s = _wh(cuda, x, w, edges, H.corner(H.bins_of(edges)), flat=flat)
    _check_scale(s, w)
    assert (got <= s[:, 1:2].astype(np.uint64)).all()


# ---------------------------------------------------------------------------
# 6. the argument rules on device arrays; an empty call writes nothing
# ---------------------------------------------------------------------------

def test_argument_rules_and_empty_call(cuda):
    import torch

    lib = _lib.load()
    M, N, d = 2, 8, 2
    xs = torch.zeros((M, N, d), dtype=torch.float32, device=cuda)
    w = torch.ones((M, N), dtype=torch.float32, device=cuda)
    ed = torch.linspace(-1, 1, 2 * 92, device=cuda)
    out = torch.full((M * 91 * 91,), FILL, dtype=torch.int64, device=cuda)
    sc = torch.full((2 * M,), FILL_SCALE, dtype=torch.int64, device=cuda)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    null = C.c_void_p(0)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)

    def call(xs=p(xs), w=p(w), d=d, n_points=M, n_draws=N, bins=i32(4, 4), keep=i32(0, -1, 0, 1), n_tables=2, sc=p(sc)):
        return lib.df_draw_weighted_histograms(xs, w, d, n_points, n_draws, p(ed), bins, keep, n_tables, p(out), sc, null)

    msg = lambda: lib.df_last_error().decode()
    assert call(d=0, n_points=-1) == _lib.DF_ERR_INVALID and "1 .. 64" in msg()
    assert call(n_points=-1, n_draws=6) == _lib.DF_ERR_SHAPE
    assert call(n_draws=6, w=null) == _lib.DF_ERR_INVALID and "multiple of 4" in msg()
    assert call(w=null, n_tables=0) == _lib.DF_ERR_INVALID and "null" in msg()
    assert call(sc=null) == _lib.DF_ERR_INVALID and "null" in msg()
    assert call(w=p(w, 8), n_tables=0) == _lib.DF_ERR_INVALID and "16-byte" in msg()
    assert call(n_tables=0) == _lib.DF_ERR_UNSUPPORTED and "n_tables" in msg()
    assert call(bins=i32(4, 129)) == _lib.DF_ERR_UNSUPPORTED and "bins[1]" in msg()
    # a 91 x 91 table is refused, and the message names the request
    assert call(bins=i32(91, 91)) == _lib.DF_ERR_UNSUPPORTED
    assert "keep[1] = {0, 1}" in msg() and "8281" in msg() and "DF_WHIST_MAX_TABLE_BINS" in msg()
    assert call(bins=i32(91, 91), n_points=0) == _lib.DF_ERR_UNSUPPORTED
    # an empty call: DF_OK, the poisoned outputs keep their bytes
    assert call(n_points=0) == _lib.DF_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all() and (sc.cpu().numpy() == FILL_SCALE).all()
    with pytest.raises(_lib.UnsupportedError, match="8192"):
        dfa.hip.run_draw_weighted_histograms(xs, w, d, M, N, ed, [91, 91], [(0, 1)], out, sc)
    with pytest.raises(_lib.UnsupportedError, match="8192"):
        dfa.weighted_histograms(xs, w, [(-1.0, 1.0, 91), (-1.0, 1.0, 91)])


# ---------------------------------------------------------------------------
# 7. the Python mirrors and the chain on a flow
# ---------------------------------------------------------------------------

def test_python_mirror(cuda):
    import torch

    M, N, d = 5, 68, 3
    edges = [(-2.0, 2.0, 8), None, np.linspace(-1, 3, 6)]
    ev, bins = dfa.histogram_edges(edges, d)
    x, rng = _draws(M, N, d, ev, 9)
    w = W.weight_patterns(M, N, rng)["hostile"]
    keep = H.corner(bins)
    ref = W.blocks(x, w, ev, keep)
    e, T, _ = W.scales(w)
    for xa, wa in ((x, w), (torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda))):
        ph = dfa.weighted_histograms(xa, wa, edges)
        assert isinstance(ph, dfa.WeightedPointHistograms) and sorted(ph.tables) == sorted(keep)
        np.testing.assert_array_equal(ph.e, e)
        np.testing.assert_array_equal(ph.T, T)
        np.testing.assert_array_equal(ph.sums(0), ref[:, :8])
        np.testing.assert_array_equal(ph.sums((0, 2)), ref[:, 13:].reshape(M, 5, 8).transpose(0, 2, 1))
        assert ph.sums((0, 2)).dtype == np.uint64
        np.testing.assert_array_equal(ph.inside(2), ref[:, 8:13].sum(axis=1, dtype=np.uint64))
        np.testing.assert_array_equal(ph.mass(0), np.ldexp(ref[:, :8].astype(np.float64), (e - 32).astype(np.int32)[:, None]))
        ok = T > 0
        np.testing.assert_allclose((ph.density(0)[ok] * np.diff(ev[0].astype(np.float64))).sum(axis=1),
                                   ph.inside(0)[ok] / T[ok], rtol=1e-14)
        assert np.isnan(ph.density(0)[~ok]).all() and (~ok).any()
        np.testing.assert_allclose(ph.pooled(2), (ref[ok, 8:13] / T[ok, None].astype(np.float64)).sum(axis=0), rtol=1e-14)


@pytest.mark.parametrize("name,M,N", [("readme", 8, 64), ("cfg2", 2, 260)])
def test_importance_posterior_histograms_on_a_flow(cuda, name, M, N):
    import torch

    flow = _flow(name)
    d, n = flow.d, flow.n
    seed, offset = 515, 4
    th = _inputs(d, n, M)[1] if n else None
    kw = dict(n_draws=N, dims=(M,), seed=seed, offset=offset)
    qt, lqt = dfa.posterior_draws(flow, th, as_tensor=True, **kw)
    calls = []

    def log_target(draws, theta):                # log q plus a Gaussian: the weights come from the Gaussian
        calls.append(tuple(draws.shape))
        assert isinstance(draws, torch.Tensor) and draws.device.type == "cuda"
        return lqt - 0.5 * ((draws - 0.25) ** 2).sum(dim=-1)

    edges = [np.linspace(-3.0 - 0.1 * (k % 3), 3.0 + 0.2 * (k % 5), 9).astype(np.float32) for k in range(d)]
    ph, iw = dfa.importance_posterior_histograms(flow, th, log_target, edges=edges, **kw)
    assert calls == [(M, N, d)] and ph.dims == (M,) and ph.n_draws == N
    # the three chained calls made by hand, bit for bit
    iw2 = dfa.importance_weights(log_target(qt, th), lqt)
    by_hand = dfa.weighted_histograms(qt, iw2, edges)
    np.testing.assert_array_equal(_bits(iw.w.cpu().numpy()), _bits(iw2.w.cpu().numpy()))
    assert sorted(ph.tables) == sorted(by_hand.tables)
    for K in ph.tables:
        np.testing.assert_array_equal(ph.sums(K), by_hand.sums(K))
    np.testing.assert_array_equal(ph.T, by_hand.T)
    np.testing.assert_array_equal(ph.e, by_hand.e)
    # and the reference on the device's own draws and weights
    x, w = qt.cpu().numpy(), iw.w.cpu().numpy()
    keep = H.corner(H.bins_of(edges))
    ref = W.blocks(x, w, edges, keep)
    np.testing.assert_array_equal(ph.sums(0), ref[:, :8])
    np.testing.assert_array_equal(ph.sums((0, 1)).transpose(0, 2, 1).reshape(M, 64), ref[:, 8 * d:8 * d + 64])
    print(f"{name} (untrained), point 0, dimension 0: weighted mass fractions {np.round(ph.sums(0)[0] / ph.T[0], 3)}, "
          f"ESS {iw.ess[0]:.1f} of {N}")
