"""GPU tests of the resampling call (df_resample.hip): df_draw_resample and its Python mirror
resample_indices / resample / importance_resample.

Everything is exact: every comparison with the pure-integer host reference (tests/resample_ref.py)
is ``==`` on the indices and on the bits of the gathered rows.  Synthetic numpy draws and weights
unless a flow is named.  Shapes (M points, N draws, d, K picks): N in {4, 12, 64, 68, 256, 260,
1028, 4096, 4100, 8196} — a wave per point with one lane, a partial wave, the wave limit (256) and
a workgroup's partial trip past it, two trips, the LDS limit (4096) and the first size past it
(the two-kernel path), two trips and a partial third of the streamed scan; K in {4, N, 1028, 2052}
— one partial tile, 17 and 33 tiles with a partial last one, tile groups of the pick kernel partly
filled; d in {1, 5, 7, 33, 61}, d = 5 at every N and every d at N in {12, 260, 4100}; M in
{1, 5, 9, 33} at N in {12, 260} — the last workgroup of the wave mapping partly filled.

Flows are untrained: ESS and the unique-pick fraction are printed, not asserted.  Flow batches
stay below the small-kernel crossover, so the bitwise comparisons stay inside one chain-pass
kernel family.
"""

import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd.data import MetaData
from densityflows_amd.hip import run_draw_resample
from helpers import spec_to_element
import resample_ref as R
from test_gpu_moments import _bounds
from test_gpu_score import _spec
from test_gpu_train import _inputs

pytestmark = pytest.mark.gpu

GUARD = 8
TAIL = 64                       # NaN floats behind every input: they must reach nothing
NAN_BITS = 0x7fc00000

NS = (4, 12, 64, 68, 256, 260, 1028, 4096, 4100, 8196)
DS = (1, 5, 7, 33, 61)
MS = (1, 5, 9, 33)
CASES = sorted({(5, N, 5) for N in NS} | {(5, N, d) for N in (12, 260, 4100) for d in DS} |
               {(M, N, 5) for M in MS for N in (12, 260)})
METHODS = ("systematic", "stratified", "multinomial")
SEED, OFFSET = 0x9e3779b97f4a7c15, 40


def _ks(N):
    return sorted({4, N, 1028, 2052})


def _per_point(method, K):
    """The Philox counters a point consumes."""
    return {"systematic": 1, "stratified": K // 4, "multinomial": K // 2}[method]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _input(a, cuda):
    """A float32 array as a flat device tensor followed by TAIL NaN floats → the tensor's head."""
    import torch

    flat = np.ascontiguousarray(a, np.float32).ravel()
    buf = torch.full((flat.size + TAIL,), np.nan, dtype=torch.float32, device=cuda)
    buf[:flat.size] = torch.from_numpy(flat).to(cuda)
    return buf[:flat.size] if flat.size else buf


def _call(cuda, q, w, K, method, seed=SEED, offset=OFFSET, want_xs=True, want_idx=True, at=None):
    """One df_draw_resample call on numpy draws (M, N, d) (None: xs = NULL, d = 0) and weights
    (M, N) → (rows (M, K, d) float32, idx (M, K) int32), None for what was not asked for.  Both
    outputs are followed by GUARD elements that must survive.  ``at``: the call covers point ``at``
    alone, with the pointers advanced and the offset advanced by the counters of the points before."""
    import torch

    M, N = w.shape
    d = q.shape[2] if q is not None else 0
    xs = _input(q, cuda) if q is not None else None
    wb = _input(w, cuda)
    out = torch.full((M * K * d + GUARD,), np.nan, dtype=torch.float32, device=cuda) if want_xs else None
    idx = torch.full((M * K + GUARD,), -7, dtype=torch.int32, device=cuda) if want_idx else None
    ws = torch.zeros(M * N, dtype=torch.int64, device=cuda) if N > dfa.RESAMPLE_LDS_DRAWS else None
    code = R.METHODS[method]
    if at is None:
        run_draw_resample(xs, wb, d, M, N, K, code, seed, offset, out, idx, ws)
    else:
        run_draw_resample(xs[at * N * d:] if xs is not None else None, wb[at * N:], d, 1, N, K, code, seed,
                          offset + at * _per_point(method, K), out[at * K * d:] if want_xs else None,
                          idx[at * K:] if want_idx else None, ws[at * N:] if ws is not None else None)
    torch.cuda.synchronize()
    res = [None, None]
    if want_xs:
        v = out.cpu().numpy()
        assert np.all(_bits(v[M * K * d:]) == NAN_BITS), "xs_out written past n_points · n_out rows"
        res[0] = v[:M * K * d].reshape(M, K, d).copy()
    if want_idx:
        v = idx.cpu().numpy()
        assert np.all(v[M * K:] == -7), "idx_out written past n_points · n_out"
        res[1] = v[:M * K].reshape(M, K).copy()
    return tuple(res)


def _weights(M, N):
    """Weights exp(logw − max) with the log-weights spread over 100 units — most of them are below
    2^−33 of the largest and quantise to 0 — one exact 0 and one duplicate of the maximum per point."""
    rng = np.random.default_rng(1000 * M + N)
    lw = rng.uniform(-100.0, 0.0, (M, N))
    w = np.exp(lw - lw.max(axis=1, keepdims=True)).astype(np.float32)
    top = np.argmax(w, axis=1)
    rows = np.arange(M)
    w[rows, (top + 1) % N] = 0.0
    w[rows, (top + 2) % N] = w[rows, top]
    return w


def _draws(M, N, d):
    rng = np.random.default_rng(7 * M + 11 * N + 13 * d)
    return (rng.standard_normal((M, N, d)) * rng.uniform(0.5, 3.0, d) + rng.uniform(-5.0, 100.0, d)).astype(np.float32)


_REF = {}


def _ref(w_key, w, K, method, seed=SEED, offset=OFFSET):
    """The reference picks, computed once per (weights, K, method) and shared, never modified."""
    key = (w_key, K, method, seed, offset)
    if key not in _REF:
        _REF[key] = R.picks(w, K, method, seed, offset)
    return _REF[key]


# ---------------------------------------------------------------------------
# 1. the picks and the gathered rows against the integer reference
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("M,N,d", CASES)
def test_picks_equal_reference(cuda, M, N, d, method):
    w, q = _weights(M, N), _draws(M, N, d)
    for K in _ks(N):
        ref = _ref((M, N), w, K, method)
        rows, idx = _call(cuda, q, w, K, method)
        np.testing.assert_array_equal(idx, ref)
        np.testing.assert_array_equal(_bits(rows), _bits(R.gather(q, ref)))
        assert np.all(idx >= 0) and np.all(idx < N)
        assert np.all(np.take_along_axis(w, idx.astype(np.int64), axis=1) > 0)
        if method != "multinomial":
            assert np.all(np.diff(idx, axis=1) >= 0)
    print(f"M={M} N={N} d={d} {method}: weights above 0 after quantising "
          f"{[sum(v > 0 for v in R.quantise(w[i])) for i in range(min(M, 3))]}, unique picks at K={K} "
          f"{[len(np.unique(idx[i])) for i in range(min(M, 3))]}")


# ---------------------------------------------------------------------------
# 2. unit weights
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N", NS)
def test_unit_weights_identity(cuda, N):
    """Systematic picks at unit weights: K = N returns xs bit for bit, K = 2N every row twice."""
    M, d = 5, 5
    q, w = _draws(M, N, d), np.ones((M, N), np.float32)
    rows, idx = _call(cuda, q, w, N, "systematic")
    np.testing.assert_array_equal(idx, np.tile(np.arange(N, dtype=np.int32), (M, 1)))
    np.testing.assert_array_equal(_bits(rows), _bits(q))
    rows, idx = _call(cuda, q, w, 2 * N, "systematic")
    np.testing.assert_array_equal(idx, np.tile(np.arange(2 * N, dtype=np.int32) // 2, (M, 1)))
    np.testing.assert_array_equal(_bits(rows), _bits(np.repeat(q, 2, axis=1)))


# ---------------------------------------------------------------------------
# 3. either output alone; guards and tails
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N,d", [(12, 5), (260, 7), (4100, 5)])
def test_outputs_optional_and_guarded(cuda, N, d, method):
    """Picks only (xs = NULL, d = 0), draws only, both: the same bits.  The guards behind every
    output and the NaN region behind every input are checked in the helper: the results hold no
    NaN, so the tails reached nothing."""
    M, K = 5, 1028
    w, q = _weights(M, N), _draws(M, N, d)
    rows, idx = _call(cuda, q, w, K, method)
    _, only_idx = _call(cuda, None, w, K, method, want_xs=False)
    only_rows, _ = _call(cuda, q, w, K, method, want_idx=False)
    _, idx_with_xs = _call(cuda, q, w, K, method, want_xs=False)       # xs given, not looked at
    np.testing.assert_array_equal(only_idx, idx)
    np.testing.assert_array_equal(idx_with_xs, idx)
    np.testing.assert_array_equal(_bits(only_rows), _bits(rows))
    np.testing.assert_array_equal(idx, _ref((M, N), w, K, method))
    assert not np.any(np.isnan(rows))


# ---------------------------------------------------------------------------
# 4. reproducible, independent of the other points
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("M,N,d", [(5, 12, 5), (5, 68, 5), (5, 260, 5), (9, 12, 61), (5, 4100, 5), (5, 8196, 5)])
def test_independent_of_points_and_path(cuda, M, N, d, method):
    """Two calls give the same bytes; point a computed alone, with the pointers advanced and the
    offset advanced by the stated counter count, gives the whole call's rows for a and leaves the
    other points' outputs alone."""
    K = 1028
    w, q = _weights(M, N), _draws(M, N, d)
    rows, idx = _call(cuda, q, w, K, method)
    rows2, idx2 = _call(cuda, q, w, K, method)
    np.testing.assert_array_equal(idx2, idx)
    np.testing.assert_array_equal(_bits(rows2), _bits(rows))
    for a in (1, M - 1):
        ra, ia = _call(cuda, q, w, K, method, at=a)
        np.testing.assert_array_equal(ia[a], idx[a])
        np.testing.assert_array_equal(_bits(ra[a]), _bits(rows[a]))
        assert np.all(np.delete(ia, a, axis=0) == -7) and np.all(np.isnan(np.delete(ra, a, axis=0)))
    # another offset, another seed: other words
    _, other = _call(cuda, None, w, K, method, offset=OFFSET + M * _per_point(method, K), want_xs=False)
    _, other_seed = _call(cuda, None, w, K, method, seed=SEED + 1, want_xs=False)
    np.testing.assert_array_equal(other, R.picks(w, K, method, SEED, OFFSET + M * _per_point(method, K)))
    np.testing.assert_array_equal(other_seed, R.picks(w, K, method, SEED + 1, OFFSET))


# ---------------------------------------------------------------------------
# 5. weights that take no part stay in their point
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", [12, 260, 4100])
def test_nonfinite_weights_stay_in_their_point(cuda, N, method):
    M, d, K = 6, 5, 1028
    w, q = _weights(M, N), _draws(M, N, d)
    rows, idx = _call(cuda, q, w, K, method)
    bad = w.copy()
    top = int(np.argmax(w[1]))
    spots = [(top + s) % N for s in (3, 4, 5, 6, 7)]
    bad[1, spots] = [np.nan, np.inf, -1.0, 1e-42, -np.inf]          # (1e-42: a subnormal beside a maximum of 1)
    bad[2, :] = 0.0
    bad[2, ::2] = -0.0
    bad[3, :] = np.nan
    rng = np.random.default_rng(N)
    bad[5, :] = rng.integers(1, 1 << 23, N).astype(np.uint32).view(np.float32)   # every weight subnormal
    rb, ib = _call(cuda, q, bad, K, method)
    ref = R.picks(bad, K, method, SEED, OFFSET)
    np.testing.assert_array_equal(ib, ref)
    np.testing.assert_array_equal(_bits(rb), _bits(R.gather(q, ref)))
    assert np.all(ib >= -1) and np.all(ib < N)
    for i in (0, 4):                                                 # the clean points, bit for bit
        np.testing.assert_array_equal(ib[i], idx[i])
        np.testing.assert_array_equal(_bits(rb[i]), _bits(rows[i]))
    assert not np.any(np.isin(ib[1], spots)), "an excluded draw was picked"
    for i in (2, 3):                                                 # the dead points
        assert np.all(ib[i] == -1) and np.all(_bits(rb[i]) == NAN_BITS)
    assert np.all(ib[5] >= 0) and len(np.unique(ib[5])) > 1
    # the dirty point's picks do not depend on what its excluded draws hold
    zeroed = bad.copy()
    zeroed[1, spots] = 0.0
    _, iz = _call(cuda, None, zeroed, K, method, want_xs=False)
    np.testing.assert_array_equal(iz, ib)


# ---------------------------------------------------------------------------
# 6. the composition the call exists for
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
def test_feeds_existing_calls(cuda, method):
    import torch

    M, N, d, K = 5, 260, 5, 1028
    q = _draws(M, N, d)
    rng = np.random.default_rng(3)
    w = np.exp(rng.uniform(-6.0, 0.0, (M, N))).astype(np.float32)
    res, idx = dfa.resample(q, w, n_out=K, method=method, seed=SEED, offset=OFFSET, return_indices=True)
    assert isinstance(res, np.ndarray) and res.shape == (M, K, d) and res.dtype == np.float32
    assert idx.shape == (M, K) and idx.dtype == np.int32
    ref_idx = R.picks(w, K, method, SEED, OFFSET)
    ref = R.gather(q, ref_idx)
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(_bits(res), _bits(ref))
    np.testing.assert_array_equal(dfa.resample_indices(w, n_out=K, method=method, seed=SEED, offset=OFFSET), ref_idx)
    # tensors in, tensors out, the same bits; n_out defaults to N
    rt = dfa.resample(torch.from_numpy(q).to(cuda), torch.from_numpy(w).to(cuda), n_out=K, method=method, seed=SEED,
                      offset=OFFSET)
    assert isinstance(rt, torch.Tensor) and rt.device.type == "cuda" and tuple(rt.shape) == (M, K, d)
    np.testing.assert_array_equal(_bits(rt.cpu().numpy()), _bits(ref))
    assert dfa.resample(q, w, method=method, seed=SEED).shape == (M, N, d)
    # order statistics: np.partition of the reference-resampled draws
    orders = [int(o) for o in dfa.quantile_orders((0.16, 0.5, 0.84), K)[0]] + [0, K - 1]
    got = dfa.order_statistics(rt, orders).cpu().numpy()
    want = np.partition(ref, sorted(set(orders)), axis=1)[:, orders, :]
    np.testing.assert_array_equal(_bits(got), _bits(want.transpose(0, 2, 1)))
    # histograms: np.histogram / np.histogram2d of the same
    spec = [(-10.0, 110.0, 16), None, (-10.0, 110.0, 8), None, None]
    ev, _ = dfa.histogram_edges(spec, d)
    tables = dfa.draw_histograms(rt, spec)
    for i in range(M):
        np.testing.assert_array_equal(tables[(0,)][i].cpu().numpy(), np.histogram(ref[i, :, 0], ev[0])[0])
        np.testing.assert_array_equal(tables[(2,)][i].cpu().numpy(), np.histogram(ref[i, :, 2], ev[2])[0])
        h2, _, _ = np.histogram2d(ref[i, :, 0], ref[i, :, 2], (ev[0], ev[2]))
        np.testing.assert_array_equal(tables[(0, 2)][i].cpu().numpy(), h2)
    # unit weights: the moments of the resampled draws
    st = dfa.weighted_stats(rt, torch.ones((M, K), dtype=torch.float32, device=cuda))
    np.testing.assert_array_equal(st.ess, np.full(M, float(K)))
    np.testing.assert_allclose(st.mean, ref.astype(np.float64).mean(axis=1).T, rtol=1e-12)
    print(f"{method}: unique fraction {[len(np.unique(idx[i])) / K for i in range(M)]}")


# ---------------------------------------------------------------------------
# 7. the pipeline on a flow
# ---------------------------------------------------------------------------

def _flow(name):
    spec, d, n = _spec(name)
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, *_bounds(n)))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,M,N,K", [("readme", 8, 64, 128), ("cfg2", 2, 260, 260)])
def test_importance_resample_on_a_flow(cuda, name, M, N, K, method):
    import torch

    flow = _flow(name)
    d, n = flow.d, flow.n
    seed, offset = 515, 4
    th = _inputs(d, n, M)[1] if n else None
    kw = dict(n_draws=N, dims=(M,), seed=seed, offset=offset)
    qt, lqt = dfa.posterior_draws(flow, th, as_tensor=True, **kw)
    calls = []

    def log_target(draws, theta):                # log q plus a quadratic: the weights come from the quadratic
        calls.append(tuple(draws.shape))
        assert isinstance(draws, torch.Tensor) and draws.device.type == "cuda"
        return lqt - 0.5 * ((draws - 0.25) ** 2).sum(dim=-1)

    out, iw = dfa.importance_resample(flow, th, log_target, n_out=K, method=method, **kw)
    assert calls == [(M, N, d)]
    assert isinstance(out, np.ndarray) and out.shape == (M, K, d) and out.dtype == np.float32
    # the composition of the four calls made by hand, bit for bit
    iw2 = dfa.importance_weights(log_target(qt, th), lqt)
    out2, idx2 = dfa.resample(qt, iw2, n_out=K, method=method, seed=seed, offset=offset, return_indices=True)
    np.testing.assert_array_equal(_bits(iw.w.cpu().numpy()), _bits(iw2.w.cpu().numpy()))
    np.testing.assert_array_equal(_bits(out), _bits(out2.cpu().numpy()))
    # the picks are the reference's on the device's own weights; the rows are rows of posterior_draws
    w = iw.w.cpu().numpy()
    ref_idx = R.picks(w, K, method, seed, offset)
    np.testing.assert_array_equal(idx2.cpu().numpy(), ref_idx)
    q = dfa.posterior_draws(flow, th, return_logpdf=False, **kw)
    np.testing.assert_array_equal(_bits(out), _bits(R.gather(q, ref_idx)))
    ot, _ = dfa.importance_resample(flow, th, log_target, n_out=K, method=method, as_tensor=True, **kw)
    assert isinstance(ot, torch.Tensor) and ot.device.type == "cuda"
    np.testing.assert_array_equal(_bits(ot.cpu().numpy()), _bits(out))
    print(f"{name} (untrained) {method}: ESS {iw.ess}, unique fraction "
          f"{[len(np.unique(ref_idx[i])) / K for i in range(M)]}")
