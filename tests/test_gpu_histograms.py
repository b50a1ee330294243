"""GPU tests of the histogram calls (df_hist.hip): df_draw_histograms, df_flow_point_histograms
and their Python mirrors draw_histograms / posterior_histograms.

Counts are integers: every comparison with the host reference (tests/histogram_ref.py:
np.histogram / np.histogram2d of the same Float32 draws — the synthetic draws given, or the
call's own draws_out) is bit for bit, and no tolerance appears anywhere.  Where a case has too
many (point, table) pairs for a numpy call each (the corners at d = 32 and 61, 257 points) the
reference is histogram_ref.blocks_indexed, which tests/test_histograms_host.py holds equal to
the numpy wrappers.

Every output buffer is pre-filled with a sentinel no count can equal (negative) and followed
by GUARD words that must survive: everything is written and nothing past the end is.

The kernel has three mappings by N = n_draws: a wave per point up to 256, a workgroup per point
up to S = HIST_SPLIT_DRAWS, and above S a point's draws divided among ceil(N / S) workgroups
whose tables merge with integer atomic adds.  (2, 256), (2, 260), (2, S), (2, S + 4) stand on the
two cutoffs.  A table past a quarter of the LDS budget (above 4096 words: 128 x 128, 128 x 33)
takes the workgroup mapping at every N.  The corner at 8 bins fits one launch up to d = 16; at
d = 32 and 61 it is walked in several groups of tables.

Chains and kernel families: those of tests/test_gpu_point_stats.py; every batch of the flow
tests lies below the README-class chain's small-kernel crossover, as that file explains.

No test states a statistical claim: the models are untrained.  The corner of one point is
printed.
"""
import numpy as np
import pytest

import densityflows_amd as dfa
from helpers import close
import histogram_ref as H
import point_stats_ref as P
from test_gpu_moments import _bounds, _chain
from test_gpu_point_stats import GUARD, INT32_MIN, _any_chain, _bits, _flow, _stats
from test_gpu_train import _dev, _inputs

pytestmark = pytest.mark.gpu

FILL = -0x12345678            # no count is negative
S = dfa.HIST_SPLIT_DRAWS
WAVE_MAX = 256                # the last N of the wave mapping


def _ref(q, edges, keep):
    return H.blocks(q, edges, keep) if q.shape[0] * len(keep) <= 400 else H.blocks_indexed(q, edges, keep)


def _count(cuda, q, edges, keep, fill=FILL, flat=None):
    """One df_draw_histograms call on numpy draws (M, N, d) → (M, T) int32.  ``flat``: the edges
    array as the device gets it (default: the edges one after the other)."""
    import torch

    M, N, d = q.shape
    bins = H.bins_of(edges)
    T = sum(H.sizes(keep, bins))
    xs = torch.from_numpy(np.ascontiguousarray(q)).to(cuda)
    eb = torch.from_numpy(H.flat_edges(edges) if flat is None else np.asarray(flat, np.float32)).to(cuda)
    out = torch.full((M * T + GUARD,), fill, dtype=torch.int32, device=cuda)
    out[M * T:] = INT32_MIN
    dfa.hip.run_draw_histograms(xs, d, M, N, eb, bins, keep, out)
    torch.cuda.synchronize()
    v = out.cpu().numpy()
    assert np.all(v[M * T:] == INT32_MIN), "counts_out written past n_points · T"
    assert np.all(v[:M * T] != fill), "counts_out not fully written"
    return v[:M * T].reshape(M, T).copy()


def _point(h, cuda, th, M, N, edges, keep, chunk=0, seed=77, offset=3, counts=True, draws=True, fill=FILL):
    """One df_flow_point_histograms call on numpy θ (n, M) → (counts (M, T) int32, draws
    (M, N, d) float32), None for what was not asked for."""
    import torch

    d, n = h.d, th.shape[0]
    bins = H.bins_of(edges)
    T = sum(H.sizes(keep, bins))
    eb = torch.from_numpy(H.flat_edges(edges)).to(cuda)
    cbuf = torch.full((M * T + GUARD,), fill, dtype=torch.int32, device=cuda) if counts else None
    if counts:
        cbuf[M * T:] = INT32_MIN
    dbuf = torch.full((d * M * N + GUARD,), np.nan, dtype=torch.float32, device=cuda) if draws else None
    h.run_point_histograms(_dev(th, cuda) if n and M else None, M, N, chunk, seed, offset, eb if counts else None,
                           bins if counts else None, keep if counts else None, cbuf, dbuf)
    torch.cuda.synchronize()
    out = [None, None]
    if counts:
        v = cbuf.cpu().numpy()
        assert np.all(v[M * T:] == INT32_MIN), "counts_out written past n_points · T"
        assert np.all(v[:M * T] != fill), "counts_out not fully written"
        out[0] = v[:M * T].reshape(M, T).copy()
    if draws:
        v = dbuf.cpu().numpy()
        assert np.all(np.isnan(v[d * M * N:])), "draws_out written past d · n_points · n_draws"
        out[1] = v[:d * M * N].reshape(M, N, d).copy()
    return tuple(out)


def _edges8(d, bins=8):
    """Per dimension `bins` equal bins on a range of its own."""
    return [np.linspace(-2.0 - 0.03 * k, 2.0 + 0.05 * k, bins + 1).astype(np.float32) for k in range(d)]


# ---------------------------------------------------------------------------
# 1. df_draw_histograms against numpy, bit for bit, on the mapping edges
# ---------------------------------------------------------------------------

# The mapping edges of the per-point kernels (tests/test_gpu_point_stats.py) — N = 4 and 12 (most
# lanes of a wave past the point's last draw), 64, 68, the last N of the wave mapping (256) and
# the first of the workgroup mapping (260: the fifth tile is 4 rows of wave 0), 4100 (past S:
# several workgroups for a point, the last with 4 rows), 257 points past one workgroup of 4 —
# and, with M = 2, both cutoffs and the cutoffs + 4.
SHAPES = [(1, 4), (3, 12), (17, 64), (5, 68), (3, 256), (3, 260), (257, 4), (2, 4100), (2, WAVE_MAX),
          (2, WAVE_MAX + 4), (2, S), (2, S + 4)]
DIMS = [1, 5, 8, 32, 61]


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_draw_histograms_exact(cuda, d, M, N):
    rng = np.random.default_rng(1000 * d + N + M)
    edges = _edges8(d)
    q = H.plant(rng.standard_normal((M, N, d)).astype(np.float32), edges, rng)
    keep = H.corner(H.bins_of(edges))
    assert len(keep) == d + d * (d - 1) // 2
    got = _count(cuda, q, edges, keep)
    ref = _ref(q, edges, keep)
    np.testing.assert_array_equal(got, ref)
    assert got.min() >= 0 and got[:, :8].sum(axis=1).max() <= N


# ---------------------------------------------------------------------------
# 2. bin shapes
# ---------------------------------------------------------------------------

def _shape_cases():
    f = np.float32
    one, big = np.array([-0.5, 0.75], f), np.linspace(-3, 3, 129).astype(f)
    uneq = np.array([-4, -1, -0.875, 0, 1e-3, 0.5, 3], f)
    zero, infs = np.array([-1, 0.0, 1], f), np.array([-np.inf, -1, 0.25, np.inf], f)
    mixed = [one, big, uneq, zero, infs]                     # L = 1, 128, unequal, an edge at +0, infinite outer edges
    big2 = np.linspace(-2.5, 2, 129).astype(f)
    corner = H.corner(H.bins_of(mixed))
    return {
        "every shape, corner": (mixed, corner),
        "one 128 x 128 table alone": ([None, big, None, big2, None], [(1, 3)]),
        "1-D tables only": (mixed, [K for K in corner if len(K) == 1]),
        "2-D tables only": (mixed, [K for K in corner if len(K) == 2]),
        "scrambled request order": (mixed, [(2, 4), (0,), (1, 3), (4,), (0, 1), (3,), (0, 4), (1,)]),
        "a dimension without bins": ([uneq, None, zero, infs, one], [(4,), (0, 2), (3,), (2, 4), (0, 3)]),
    }


@pytest.mark.parametrize("M,N", [(3, 260), (3, 12)])
@pytest.mark.parametrize("name", list(_shape_cases()))
def test_bin_shapes(cuda, name, M, N):
    """(3, 260): a workgroup per point.  (3, 12): a wave per point, and a workgroup per point
    where a table is past a wave's share of the LDS (the 128-bin cases)."""
    edges, keep = _shape_cases()[name]
    rng = np.random.default_rng(N + len(keep))
    q = H.plant(rng.standard_normal((M, N, 5)).astype(np.float32), edges, rng)
    got = _count(cuda, q, edges, keep)
    np.testing.assert_array_equal(got, H.blocks(q, edges, keep))


# ---------------------------------------------------------------------------
# 3. the split path
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d,M,N", [(5, 2, S - 4), (5, 2, S), (5, 2, S + 4), (5, 2, 2 * S + 4), (32, 2, S + 4),
                                   (5, 257, S + 4)])
def test_split_path(cuda, d, M, N):
    """N <= S: one workgroup per point, plain stores.  Above: ceil(N / S) workgroups per point,
    the last with 4 draws, integer atomic adds into blocks the call zeroes: the same counts, and
    the same bytes from two calls into differently pre-filled buffers."""
    rng = np.random.default_rng(d + N + M)
    edges = _edges8(d)
    q = H.plant(rng.standard_normal((M, N, d)).astype(np.float32), edges, rng)
    keep = H.corner(H.bins_of(edges))
    a = _count(cuda, q, edges, keep)
    b = _count(cuda, q, edges, keep, fill=-7)
    np.testing.assert_array_equal(a, _ref(q, edges, keep))
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# 4. hostile edges stay in bounds
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["unsorted", "all equal", "NaN"])
def test_hostile_edges_stay_in_bounds(cuda, kind):
    """The C call does not read the edges; its search is bounded by construction (the step
    guard and the clamped read of df_hist.hip), so that for any edge content every add lands in
    the point's own block or is dropped.  Checked here on memory the call owns: the guards
    survive, every word is written, every count lies in [0, N].  Nothing else is asserted."""
    M, N, d = 3, 68, 5
    rng = np.random.default_rng(17)
    edges = _edges8(d)
    q = H.plant(rng.standard_normal((M, N, d)).astype(np.float32), edges, rng)
    flat = H.flat_edges(edges)
    if kind == "unsorted":
        flat = rng.permutation(flat)
    elif kind == "all equal":
        flat = np.full_like(flat, 0.25)
    else:
        flat = flat.copy()
        flat[rng.permutation(flat.size)[:flat.size // 2]] = np.nan
        flat[-1] = np.nan
    got = _count(cuda, q, edges, H.corner(H.bins_of(edges)), flat=flat)
    assert got.min() >= 0 and got.max() <= N


# ---------------------------------------------------------------------------
# 5. the flow's own draws
# ---------------------------------------------------------------------------

def _flow_edges(d):
    return [np.linspace(-3.0 - 0.1 * (k % 3), 3.0 + 0.2 * (k % 5), 9).astype(np.float32) for k in range(d)]


@pytest.mark.parametrize("M,N", [(3, 12), (5, 68), (2, 516)])
@pytest.mark.parametrize("name", ["readme", "cfg2", "wide", "norm61"])
def test_point_histograms_exact_against_own_draws(cuda, name, M, N):
    spec, d, n, h = _any_chain(name)
    x, th = _inputs(d, n, M)
    edges = _flow_edges(d)
    keep = H.corner(H.bins_of(edges))
    c, q = _point(h, cuda, th, M, N, edges, keep)
    assert np.all(np.isfinite(q)), "draws_out not fully overwritten"
    np.testing.assert_array_equal(c, _ref(q, edges, keep))
    print(f"{name}: {int(c[:, :8].sum())} of {M * N} draws of dimension 0 inside its edges")
    # the draws are df_flow_point_stats' at the same (seed, offset)
    _, _, q0 = _stats(h, cuda, x, th, N, ranks=False, sums=False)
    np.testing.assert_array_equal(_bits(q), _bits(q0))
    # the counts alone, and the draws alone (the tables are then not looked at)
    c1, _ = _point(h, cuda, th, M, N, edges, keep, draws=False)
    np.testing.assert_array_equal(c1, c)
    _, q2 = _point(h, cuda, th, M, N, edges, keep, counts=False)
    np.testing.assert_array_equal(_bits(q2), _bits(q))


# M = 7, N = 260: chunk 0 takes the 1820 draws at once, 780 three points at a time (the last
# chunk one point), 260 one point at a time.  All below the small-kernel crossover.
@pytest.mark.parametrize("name", ["readme", "cfg2"])
def test_chunking_and_other_points(cuda, name):
    spec, d, n, h = _chain(name)
    M, N, seed, offset = 7, 260, 11, 4
    x, th = _inputs(d, n, M)
    edges = _flow_edges(d)
    keep = H.corner(H.bins_of(edges))
    c, q = _point(h, cuda, th, M, N, edges, keep, seed=seed, offset=offset)
    np.testing.assert_array_equal(c, H.blocks(q, edges, keep))
    for chunk in (N, 3 * N, 0):
        cc, qc = _point(h, cuda, th, M, N, edges, keep, chunk=chunk, seed=seed, offset=offset)
        np.testing.assert_array_equal(cc, c, err_msg=f"chunk {chunk}")
        np.testing.assert_array_equal(_bits(qc), _bits(q))
    # the first K points of the call are a call of K points
    K = 3
    ck, qk = _point(h, cuda, th[:, :K], K, N, edges, keep, seed=seed, offset=offset)
    np.testing.assert_array_equal(ck, c[:K])
    np.testing.assert_array_equal(_bits(qk), _bits(q[:K]))
    # point 3 alone, at its own counter
    c3, _ = _point(h, cuda, th[:, 3:4], 1, N, edges, keep, seed=seed, offset=offset + d * 3 * N // 4)
    np.testing.assert_array_equal(c3[0], c[3])


def test_empty_call_writes_nothing(cuda):
    import torch

    spec, d, n, h = _chain("readme")
    edges = _flow_edges(d)
    keep = H.corner(H.bins_of(edges))
    _, th = _inputs(d, n, 0)
    # fill = INT32_MIN: "fully written" is vacuous for no words; the guards are every word
    c, q = _point(h, cuda, th, 0, 8, edges, keep)
    assert c.shape == (0, sum(H.sizes(keep, H.bins_of(edges)))) and q.shape == (0, 8, d)
    out = torch.full((GUARD,), INT32_MIN, dtype=torch.int32, device=cuda)
    xs = torch.zeros(16, dtype=torch.float32, device=cuda)
    eb = torch.from_numpy(H.flat_edges(edges)).to(cuda)
    dfa.hip.run_draw_histograms(xs, d, 0, 8, eb, H.bins_of(edges), keep, out)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == INT32_MIN)
    flow = _flow("readme")
    e = dfa.posterior_histograms(flow, np.zeros((n, 0), np.float32), edges=edges, n_draws=8, seed=1)
    assert e.counts[(0,)].shape == (0, 8) and e.counts[(0, 1)].shape == (0, 8, 8)
    assert dfa.draw_histograms(np.zeros((0, 8, d), np.float32), edges)[(1, 2)].shape == (0, 8, 8)


# ---------------------------------------------------------------------------
# 6. against the fp64 oracle: a derived bracket
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["readme", "cfg2", "wide", "cfg5"])
def test_against_oracle(cuda, name):
    """With δ the largest |device draw − oracle draw| of a point's dimension, a device draw in
    [e_j, e_{j+1}) has its oracle draw in [e_j − δ, e_{j+1} + δ], and an oracle draw in
    [e_j + δ, e_{j+1} − δ) has its device draw in the bin: per bin
    #{oracle in [e_j + δ, e_{j+1} − δ)} <= count <= #{oracle in [e_j − δ, e_{j+1} + δ]}, and the
    same with rectangles for a 2-D table.  A bracket that follows from δ, not a tolerance; the
    number of oracle draws in the ±δ bands is printed."""
    import torch

    spec, d, n, h = _chain(name)
    M, N, seed, offset = P.ORACLE_M, P.ORACLE_N, 2025, 1
    x, th = _inputs(d, n, M)
    edges = _flow_edges(d)
    keep = H.corner(H.bins_of(edges))
    c, q = _point(h, cuda, th, M, N, edges, keep, seed=seed, offset=offset)
    z = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    h.random_normal(z, d * M * N, seed, offset)
    torch.cuda.synchronize()
    z64 = z.cpu().numpy().reshape(M * N, d).T.astype(np.float64)
    q64 = P.oracle_draws(spec, th, z64, N, *_bounds(n))                  # (M, N, d)
    ok, rq = close(q, q64)
    assert ok, rq
    delta = np.max(np.abs(q.astype(np.float64) - q64), axis=1)           # (M, d)
    sizes = H.sizes(keep, H.bins_of(edges))
    in_band = 0
    for i in range(M):
        lo_in, up_in = [], []                                            # per dimension (N, L) membership
        for k in range(d):
            e = edges[k].astype(np.float64)
            o, dl = q64[i, :, k][:, None], delta[i, k]
            lo_in.append(((o >= e[:-1] + dl) & (o < e[1:] - dl)).astype(np.int64))
            up_in.append(((o >= e[:-1] - dl) & (o <= e[1:] + dl)).astype(np.int64))
            in_band += int(np.sum(np.any(np.abs(o - e[None, :]) <= dl, axis=1)))
        at = 0
        for K, size in zip(keep, sizes):
            got = c[i, at:at + size]
            if len(K) == 1:
                lo, up = lo_in[K[0]].sum(axis=0), up_in[K[0]].sum(axis=0)
            else:
                lo = (lo_in[K[0]].T @ lo_in[K[1]]).T.reshape(-1)          # i_a + L_a · i_b
                up = (up_in[K[0]].T @ up_in[K[1]]).T.reshape(-1)
            assert np.all(lo <= got) and np.all(got <= up), (i, K)
            at += size
    print(f"{name}: draws parity {rq:.3f}; largest δ {delta.max():.3e}; {in_band} of {M * N * d} oracle "
          f"coordinates lie within δ of an edge; {int(c[:, :8].sum())} of {M * N} draws of dimension 0 inside")


# ---------------------------------------------------------------------------
# 7. Python
# ---------------------------------------------------------------------------

def test_posterior_histograms(cuda):
    import torch

    flow = _flow("readme")
    d, n, dims, N, seed = 5, 1, (2, 5, 7), 64, 19
    M = 70
    _, th = _inputs(d, n, M)
    tha = np.asfortranarray(th).reshape((n,) + dims, order="F")
    spec = [(-3.0, 3.0, 8), np.array([-4, -1, 0, 0.5, 4], np.float32), None, (-2.5, 2.5, 5), [-np.inf, 0.0, np.inf]]
    ph, draws = dfa.posterior_histograms(flow, tha, edges=spec, n_draws=N, seed=seed, return_draws=True)
    assert isinstance(ph, dfa.PointHistograms) and ph.n_draws == N and ph.dims == dims
    assert draws.shape == (M, N, d) and draws.dtype == np.float32
    ev, bins = dfa.histogram_edges(spec, d)
    np.testing.assert_array_equal(bins, [8, 4, 0, 5, 2])
    np.testing.assert_array_equal(ev[0], np.linspace(-3.0, 3.0, 9).astype(np.float32))
    keys = H.corner(bins)
    assert list(ph.counts) == keys and len(keys) == 4 + 6
    ref = H.blocks(draws, ev, keys)
    at = 0
    for K, size in zip(keys, H.sizes(keys, bins)):
        t = ph.counts[K]
        assert t.dtype == np.int32 and t.shape == (M,) + tuple(int(bins[k]) for k in K)
        want = ref[:, at:at + size]
        if len(K) == 2:
            want = want.reshape(M, bins[K[1]], bins[K[0]]).transpose(0, 2, 1)
            h2, _, _ = np.histogram2d(draws[3, :, K[0]], draws[3, :, K[1]], (ev[K[0]], ev[K[1]]))
            np.testing.assert_array_equal(t[3], h2)                       # np.histogram2d's own shape
        np.testing.assert_array_equal(t, want)
        at += size
        # inside, density, pooled
        np.testing.assert_array_equal(ph.inside(K), t.reshape(M, -1).sum(axis=1))
        np.testing.assert_array_equal(ph.pooled(K), t.astype(np.int64).sum(axis=0))
        w = np.diff(ev[K[0]].astype(np.float64))
        if len(K) == 2:
            w = w[:, None] * np.diff(ev[K[1]].astype(np.float64))[None, :]
        den = ph.density(K)
        assert den.dtype == np.float64 and den.shape == t.shape
        fin = np.isfinite(w)
        integral = np.where(fin, den * np.where(fin, w, 1.0), 0.0).reshape(M, -1).sum(axis=1)
        inside_fin = np.where(fin, t, 0).reshape(M, -1).sum(axis=1)
        np.testing.assert_allclose(integral, inside_fin / N, rtol=1e-14, atol=0)
    assert np.all(ph.inside((4,)) == N)                                   # (−inf, inf) holds every draw
    # draws_out are posterior_quantiles' at the same seed
    _, d0 = dfa.posterior_quantiles(flow, tha, n_draws=N, seed=seed, return_draws=True)
    np.testing.assert_array_equal(_bits(draws), _bits(d0))
    # without the draws; device θ, chunked; an NTuple θ; a keep of its own, merged and sorted
    p1 = dfa.posterior_histograms(flow, tha, edges=spec, n_draws=N, seed=seed)
    tht = torch.from_numpy(np.ascontiguousarray(tha)).to(cuda)
    p2 = dfa.posterior_histograms(flow, tht, edges=spec, n_draws=N, seed=seed, chunk=128)
    for K in keys:
        np.testing.assert_array_equal(p1.counts[K], ph.counts[K])
        np.testing.assert_array_equal(p2.counts[K], ph.counts[K])
    a = dfa.posterior_histograms(flow, (1.25,), edges=spec, n_draws=N, dims=dims, seed=seed, keep=[(3, 0), 1, (0, 3), (1,)])
    b = dfa.posterior_histograms(flow, np.full((n,) + dims, 1.25, np.float32), edges=spec, n_draws=N, seed=seed)
    assert list(a.counts) == [(1,), (0, 3)]
    for K in a.counts:
        np.testing.assert_array_equal(a.counts[K], b.counts[K])
    # draw_histograms on the returned draws: numpy in, and a device tensor in
    h_np = dfa.draw_histograms(draws, spec)
    assert list(h_np) == keys
    h_t = dfa.draw_histograms(torch.from_numpy(draws).to(cuda), spec, keep=[(0, 1), (4,)])
    assert list(h_t) == [(4,), (0, 1)]
    for K in keys:
        assert isinstance(h_np[K], np.ndarray) and h_np[K].dtype == np.int32
        np.testing.assert_array_equal(h_np[K], ph.counts[K])
    for K, t in h_t.items():
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32
        np.testing.assert_array_equal(t.cpu().numpy(), ph.counts[K])
    # refusals
    with pytest.raises(dfa.ArgumentError, match="dimension 1"):
        dfa.posterior_histograms(flow, tha, edges=[None, [0, 0, 1], None, None, None], n_draws=N, seed=seed)
    with pytest.raises(dfa.ArgumentError, match="without edges"):
        dfa.posterior_histograms(flow, tha, edges=spec, keep=[(2,)], n_draws=N, seed=seed)
    with pytest.raises(dfa.ArgumentError, match="multiple of 4"):
        dfa.draw_histograms(draws[:, :6], spec)
    with pytest.raises(dfa.UnsupportedError):
        dfa.posterior_histograms(flow, tha, edges=spec, keep=[(0, 1, 3)], n_draws=N, seed=seed)
    # the corner of point 0
    print("readme (untrained), point 0, the corner (rows: lower dimension):")
    for K in keys:
        print(f"  {K}: inside {int(ph.inside(K)[0])} of {N}\n    " +
              str(ph.counts[K][0]).replace("\n", "\n    "))


def test_posterior_histograms_unconditional(cuda):
    """An unconditional flow with one "point" of many draws: the split path behind the Python call."""
    flow = _flow("cfg2")
    d = flow.d
    N = 2 * S + 4
    spec = [(-3.0, 3.0, 16)] * d
    ph, draws = dfa.posterior_histograms(flow, edges=spec, n_draws=N, dims=(), seed=5, return_draws=True)
    assert draws.shape == (1, N, d)
    ev, bins = dfa.histogram_edges(spec, d)
    keys = H.corner(bins)
    ref = H.blocks(draws, ev, keys)
    at = 0
    for K, size in zip(keys, H.sizes(keys, bins)):
        want = ref[:, at:at + size]
        if len(K) == 2:
            want = want.reshape(1, 16, 16).transpose(0, 2, 1)
        np.testing.assert_array_equal(ph.counts[K], want)
        at += size
    # the counts of two calls at disjoint counters add up to the counts of their draws together
    p2, d2 = dfa.posterior_histograms(flow, edges=spec, n_draws=N, dims=(), seed=5, offset=d * N // 4, return_draws=True)
    both = H.blocks(np.concatenate([draws, d2], axis=1), ev, [(0, 1)])
    np.testing.assert_array_equal((ph.counts[(0, 1)] + p2.counts[(0, 1)])[0].T.reshape(-1), both[0])
