"""GPU tests of the posterior-summary call (df_pstats.hip): df_flow_point_stats and its Python
mirror posterior_stats / sbc_ranks.

Chains: those of tests/test_gpu_hpd.py — "readme" (d 5, n 1), "cfg2" (5, 0), "wide" (8, 3) —
plus "cfg5" (d 32, n 8: 528 pair sums, 9 passes of a wave's lanes over a tile) and "norm61",
one NormalizationLayer at d = 61, n = 0 (the largest odd d, no multiple of 4, 1891 pairs, no
weights), with its smaller kin "norm13", "norm3", "norm1" for the d at which the sums change
path; θ bounds (−1, 3), points from _inputs.

Kernel families.  Every batch here — the draws of a call or of one chunk, at most
2 · 4100 = 8200 samples — lies below the README-class chain's small-kernel crossover (32768
samples on 256 CUs), so every bitwise comparison stays inside one chain-pass family.

No test states a statistical claim: the models are untrained.  Rank histograms are printed.
"""
import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd.data import MetaData
from helpers import close, spec_to_element
import point_stats_ref as P
from test_gpu_moments import _bounds, _chain
from test_gpu_score import _spec
from test_gpu_train import _dev, _inputs

pytestmark = pytest.mark.gpu

GUARD = 8
INT32_MIN = -(2 ** 31)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _any_chain(name):
    """(spec, d, n, HIPChain): _chain's, or "norm<d>", the lone NormalizationLayer at that d."""
    if name.startswith("norm"):
        d = int(name[4:])
        spec = P.norm_spec(d)
        return spec, d, 0, spec_to_element(spec).hip()
    return _chain(name)


def _stats(h, cuda, x, th, N, chunk=0, seed=77, offset=3, ranks=True, sums=True, draws=True, shift=0, M=None):
    """One df_flow_point_stats call on numpy x (d, M), θ (n, M) → (ranks (d, M) int32, blocks
    (M, S) float64, draws (M, N, d) float32), None for what was not asked for.  Every output is
    followed by GUARD elements (INT32_MIN, NaN) that must survive; ``shift``: the draws' buffer
    starts that many floats past a 16-byte boundary."""
    import torch

    d = x.shape[0]
    M = x.shape[1] if M is None else M
    n = th.shape[0]
    S = P.entries(d)
    rank = torch.full((d * M + GUARD,), INT32_MIN, dtype=torch.int32, device=cuda) if ranks else None
    sbuf = torch.full((S * M + GUARD,), np.nan, dtype=torch.float64, device=cuda) if sums else None
    dbuf = torch.full((4 + d * M * N + GUARD,), np.nan, dtype=torch.float32, device=cuda) if draws else None
    nan_bits = _bits(np.float32(np.nan).reshape(1))[0]
    # (an empty call still needs a non-null x beside rank_out: the rule is checked first)
    xb = (_dev(x, cuda) if M else torch.zeros(d, dtype=torch.float32, device=cuda)) if ranks else None
    h.run_point_stats(xb, _dev(th, cuda) if n and M else None, M, N, chunk, seed, offset, rank, sbuf,
                      dbuf[shift:] if draws else None)
    torch.cuda.synchronize()
    out = [None, None, None]
    if ranks:
        r = rank.cpu().numpy()
        assert np.all(r[d * M:] == INT32_MIN), "rank_out written past d · n_points"
        assert np.all(r[:d * M] != INT32_MIN), "rank_out not fully written"
        out[0] = r[:d * M].reshape(M, d).T.copy()
    if sums:
        v = sbuf.cpu().numpy()
        assert np.all(np.isnan(v[S * M:])), "sums_out written past n_points blocks"
        out[1] = v[:S * M].reshape(M, S).copy()
    if draws:
        v = dbuf.cpu().numpy()
        assert np.all(_bits(v[:shift]) == nan_bits) and np.all(_bits(v[shift + d * M * N:]) == nan_bits), \
            "draws_out written outside d · n_points · n_draws"
        out[2] = v[shift:shift + d * M * N].reshape(M, N, d).copy()
    return tuple(out)


# ---------------------------------------------------------------------------
# 1. exact against the call's own draws
# ---------------------------------------------------------------------------

# N draws are N rows of 64-row tiles, a lane per row.  (1, 4), (3, 12), (17, 64), (257, 4):
# several points per wave (16, 5, 1 of them), idle lanes behind the last point (12 · 5 = 60
# rows), a last wave partly filled, 257 points past one workgroup of 4 · 16.  (5, 68), (3, 256):
# a wave per point, 5 points past one workgroup, the second trip 4 rows; four full trips, the
# last N of this mapping.  (3, 260), (2, 4100), (2, 516): a workgroup per point, 5 trips (wave 0
# takes two, the second 4 rows), 65 trips, 9 trips.
SHAPES = [(1, 4), (3, 12), (17, 64), (5, 68), (3, 260), (257, 4), (2, 4100), (3, 256)]
BIG_D_SHAPES = [(3, 12), (5, 68), (2, 516)]
# The sums take another path with d (df_pstats.hip): a tile of shifted doubles up to d = 16 — one
# pass of the lanes shared by 64 / E row groups while E = d + d(d+1)/2 <= 32 (readme, cfg2: 3 groups,
# 60 lanes; norm3: 7 groups, 63 lanes; norm1: 32 groups of 2 lanes), one pass without groups (wide,
# E = 44), two passes (norm13, E = 104) — and the Float32 tile above (cfg5, norm61).
CASES = [(name, M, N) for name in ("readme", "cfg2", "wide") for M, N in SHAPES] + \
        [(name, M, N) for name in ("cfg5", "norm61", "norm13", "norm3", "norm1") for M, N in BIG_D_SHAPES]


@pytest.mark.parametrize("name,M,N", CASES)
def test_exact_against_own_draws(cuda, name, M, N):
    spec, d, n, h = _any_chain(name)
    x, th = _inputs(d, n, M)
    r, blk, q = _stats(h, cuda, x, th, N)
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(blk)), "outputs not fully overwritten"
    np.testing.assert_array_equal(r, P.ranks(x, q))
    assert r.dtype == np.int32 and np.all((0 <= r) & (r <= N))
    ref, bound = P.exact_sums(q)
    np.testing.assert_array_equal(_bits64(blk[:, :d]), _bits64(q[:, 0, :].astype(np.float64)))   # c = draw 0
    err = np.abs(blk - ref)
    worst = float(np.max(err[:, d:] / np.maximum(bound[:, d:], np.finfo(np.float64).tiny)))
    print(f"{name} M={M} N={N}: ranks {r[:, 0][:8]}, sums error / bound {worst:.3f}")
    assert np.all(err <= bound), worst
    # the other template instances return the same bits
    r2, _, _ = _stats(h, cuda, x, th, N, sums=False, draws=False)
    np.testing.assert_array_equal(r2, r)
    _, b3, _ = _stats(h, cuda, x, th, N, ranks=False, draws=False)
    np.testing.assert_array_equal(_bits64(b3), _bits64(blk))
    r4, b4, _ = _stats(h, cuda, x, th, N, draws=False)
    np.testing.assert_array_equal(r4, r)
    np.testing.assert_array_equal(_bits64(b4), _bits64(blk))
    # a draws buffer off the 16-byte boundary: the same values everywhere
    r5, b5, q5 = _stats(h, cuda, x, th, N, shift=1)
    np.testing.assert_array_equal(r5, r)
    np.testing.assert_array_equal(_bits64(b5), _bits64(blk))
    np.testing.assert_array_equal(_bits(q5), _bits(q))


# ---------------------------------------------------------------------------
# 2. the draws are the documented ones
# ---------------------------------------------------------------------------

# batches: 17 · 68 = 1156 draws in one chunk, in the df_flow_sample call and in the forward pass
@pytest.mark.parametrize("name", ["readme", "cfg2", "wide"])
def test_draws_are_sample(cuda, name):
    import torch

    spec, d, n, h = _chain(name)
    M, N, seed, offset = 17, 68, 4321, 6
    x, th = _inputs(d, n, M)
    _, _, q = _stats(h, cuda, x, th, N, seed=seed, offset=offset, ranks=False, sums=False)
    th_rep = _dev(np.repeat(th, N, axis=1), cuda) if n else None
    xs = torch.full((d * M * N,), np.nan, dtype=torch.float32, device=cuda)
    h.run_sample(xs, th_rep, False, M * N, seed, offset)
    # the base normals are random_normal's at the same counters: sent through forward!, the same samples
    z = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    h.random_normal(z, d * M * N, seed, offset)
    h.run_inplace(z, th_rep, M * N, flow=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(q.ravel()), _bits(xs.cpu().numpy()))
    np.testing.assert_array_equal(_bits(q.ravel()), _bits(z.cpu().numpy()))


# ---------------------------------------------------------------------------
# 3. independence of chunking and of the other points
# ---------------------------------------------------------------------------

# M = 7, N = 260: chunk 0 and 2^14 take the 1820 draws at once, 520 two points at a time (the
# last chunk one point), 260 and 100 (below N) one point at a time.
@pytest.mark.parametrize("name", ["readme", "cfg2"])
def test_chunking_and_other_points(cuda, name):
    spec, d, n, h = _chain(name)
    M, N, seed, offset = 7, 260, 11, 4
    x, th = _inputs(d, n, M)
    r, blk, q = _stats(h, cuda, x, th, N, seed=seed, offset=offset)
    for chunk in (260, 520, 100, 1 << 14, 0):
        rc, bc, qc = _stats(h, cuda, x, th, N, chunk=chunk, seed=seed, offset=offset)
        np.testing.assert_array_equal(rc, r, err_msg=f"chunk {chunk}")
        np.testing.assert_array_equal(_bits64(bc), _bits64(blk), err_msg=f"chunk {chunk}")
        np.testing.assert_array_equal(_bits(qc), _bits(q))
    # point 3 alone, at its own counter
    r3, b3, q3 = _stats(h, cuda, x[:, 3:4], th[:, 3:4], N, seed=seed, offset=offset + d * 3 * N // 4)
    np.testing.assert_array_equal(r3[:, 0], r[:, 3])
    np.testing.assert_array_equal(_bits64(b3[0]), _bits64(blk[3]))
    np.testing.assert_array_equal(_bits(q3[0]), _bits(q[3]))


# ---------------------------------------------------------------------------
# 4. parity with the fp64 oracle
# ---------------------------------------------------------------------------

def _oracle_checks(name, x, r, blk, q, q64, d, N):
    ok, rq = close(q, q64)
    assert ok, rq
    lo, hi = P.rank_bracket(x, q64)
    share = np.sum(hi - lo) / (d * q.shape[0] * N)
    assert np.all(lo <= r) and np.all(r <= hi), (lo, r, hi)
    mean, cov = P.moments(blk, d, N)
    om, oc = P.plain_moments(q64)
    mb, cb = P.moment_bounds(q64)
    rm, rc = float(np.max(np.abs(mean - om) / mb)), float(np.max(np.abs(cov - oc) / cb))
    print(f"{name}: draws parity {rq:.3f}; bracket share {share:.6f}; mean error / bound {rm:.3f}, "
          f"cov error / bound {rc:.3f}")
    print(f"{name}: rank histogram (dimension × 9 bins of 29)\n{dfa.sbc_histogram(r, N, 9)}")
    assert share <= P.UNDECIDED_CAP
    assert np.all(np.abs(mean - om) <= mb), rm
    assert np.all(np.abs(cov - oc) <= cb), rc


@pytest.mark.parametrize("name", ["readme", "cfg2", "wide", "cfg5"])
def test_against_oracle(cuda, name):
    """The cap Σ(hi − lo) <= 0.002 · d · M · N is a property of the samples' distribution, not of
    the Philox stream: tests/test_point_stats_host.py::test_bracket_is_tight_for_the_oracle_alone
    holds the oracle alone to it on the CPU, with numpy normal draws, for these chains, points,
    θ and (M, N).  Observed share there: readme 0, cfg2 0.000045, wide 0.000085, cfg5 0.000049."""
    import torch

    spec, d, n, h = _chain(name)
    M, N, seed, offset = P.ORACLE_M, P.ORACLE_N, 2025, 1
    x, th = _inputs(d, n, M)
    r, blk, q = _stats(h, cuda, x, th, N, seed=seed, offset=offset)
    z = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    h.random_normal(z, d * M * N, seed, offset)
    torch.cuda.synchronize()
    z64 = z.cpu().numpy().reshape(M * N, d).T.astype(np.float64)
    q64 = P.oracle_draws(spec, th, z64, N, *_bounds(n))
    _oracle_checks(name, x, r, blk, q, q64, d, N)


# ---------------------------------------------------------------------------
# 5. d = 61: the closed form of a lone NormalizationLayer
# ---------------------------------------------------------------------------

def test_norm61_closed_form(cuda):
    """x = A·z + b per dimension: the device's mean and covariance are that affine map of the
    fp64 mean and covariance of the base draw, within the bounds of the oracle test."""
    import torch

    spec, d, n, h = _any_chain("norm61")
    M, N, seed, offset = 5, 260, 99, 2
    x, th = _inputs(d, n, M)
    r, blk, q = _stats(h, cuda, x, th, N, seed=seed, offset=offset)
    z = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    h.random_normal(z, d * M * N, seed, offset)
    torch.cuda.synchronize()
    z64 = z.cpu().numpy().reshape(M, N, d).astype(np.float64)
    A, b = P.norm_affine(spec)
    zm, zc = P.plain_moments(z64)
    mean, cov = P.moments(blk, d, N)
    mb, cb = P.moment_bounds(A * z64 + b)
    em = np.abs(mean - (A[:, None] * zm + b[:, None]))
    ec = np.abs(cov - A[:, None, None] * A[None, :, None] * zc)
    print(f"norm61: mean error / bound {np.max(em / mb):.3f}, cov error / bound {np.max(ec / cb):.3f}")
    assert np.all(em <= mb) and np.all(ec <= cb)
    lo, hi = P.rank_bracket(x, A * z64 + b)
    assert np.all(lo <= r) and np.all(r <= hi)


# ---------------------------------------------------------------------------
# 6. special values
# ---------------------------------------------------------------------------

def test_special_values(cuda):
    spec, d, n, h = _chain("readme")
    M, N = 5, 260
    x, th = _inputs(d, n, M)
    r, blk, q = _stats(h, cuda, x, th, N)
    bad = x.copy()
    bad[2, 1] = np.nan
    bad[0, 3] = np.inf
    bad[4, 3] = -np.inf
    rb, bb, qb = _stats(h, cuda, bad, th, N)
    assert rb[2, 1] == 0 and rb[0, 3] == N and rb[4, 3] == 0
    np.testing.assert_array_equal(rb, P.ranks(bad, qb))
    same = np.ones((d, M), bool)
    same[2, 1] = same[0, 3] = same[4, 3] = False
    np.testing.assert_array_equal(rb[same], r[same])            # that dimension only
    # neither the draws nor the sums depend on the points
    np.testing.assert_array_equal(_bits(qb), _bits(q))
    np.testing.assert_array_equal(_bits64(bb), _bits64(blk))


def test_empty_call_writes_nothing(cuda):
    spec, d, n, h = _chain("readme")
    x, th = _inputs(d, n, 0)
    r, blk, q = _stats(h, cuda, x, th, 8, M=0)       # the guards (every element) are checked inside
    assert r.shape == (d, 0) and blk.shape == (0, P.entries(d)) and q.shape == (0, 8, d)


# ---------------------------------------------------------------------------
# 7. Python
# ---------------------------------------------------------------------------

def _flow(name):
    spec, d, n = _spec(name)
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, *_bounds(n)))


def test_posterior_stats(cuda):
    import torch

    flow = _flow("readme")
    d, n, dims, N, seed = 5, 1, (2, 5, 7), 64, 19
    M = 70
    x, th = _inputs(d, n, M)
    h = flow.hip()
    # the low-level call on the flat (Julia-order) points
    r, blk, _ = _stats(h, cuda, x, th, N, seed=seed, offset=0, draws=False)
    mean, cov = P.moments(blk, d, N)
    xa = np.asfortranarray(x).reshape((d,) + dims, order="F")
    tha = np.asfortranarray(th).reshape((n,) + dims, order="F")
    st = dfa.posterior_stats(flow, tha, n_draws=N, x=xa, seed=seed)
    assert isinstance(st, dfa.PointStats) and st.n_draws == N
    assert st.mean.shape == (d,) + dims and st.mean.dtype == np.float64
    assert st.cov.shape == (d, d) + dims and st.std.shape == (d,) + dims
    assert st.ranks.shape == (d,) + dims and st.ranks.dtype == np.int32
    np.testing.assert_array_equal(st.ranks.reshape(d, M, order="F"), r)
    np.testing.assert_array_equal(st.mean.reshape(d, M, order="F"), mean)
    np.testing.assert_array_equal(st.cov.reshape(d, d, M, order="F"), cov)
    np.testing.assert_array_equal(st.std, np.sqrt(np.stack([st.cov[k, k] for k in range(d)])))
    np.testing.assert_array_equal(st.zscore(xa), (st.mean - xa) / st.std)
    # the ranks-only call; device tensors in, chunked
    rk = dfa.sbc_ranks(flow, xa, tha, n_draws=N, seed=seed)
    assert rk.dtype == np.int32
    np.testing.assert_array_equal(rk, st.ranks)
    xt = torch.from_numpy(np.ascontiguousarray(xa)).to(cuda)
    tht = torch.from_numpy(np.ascontiguousarray(tha)).to(cuda)
    np.testing.assert_array_equal(dfa.sbc_ranks(flow, xt, tht, n_draws=N, seed=seed, chunk=128), rk)
    # without points: no ranks, the same sums
    s0 = dfa.posterior_stats(flow, tha, n_draws=N, seed=seed)
    assert s0.ranks is None
    np.testing.assert_array_equal(_bits64(s0.mean), _bits64(st.mean))
    np.testing.assert_array_equal(_bits64(s0.cov), _bits64(st.cov))
    # an NTuple θ is that θ in every column, bitwise
    one = (1.25,)
    full = np.full((n,) + dims, 1.25, np.float32)
    a = dfa.posterior_stats(flow, one, n_draws=N, x=xa, seed=seed)
    b = dfa.posterior_stats(flow, full, n_draws=N, x=xa, seed=seed)
    c = dfa.posterior_stats(flow, one, n_draws=N, dims=dims, seed=seed)
    np.testing.assert_array_equal(a.ranks, b.ranks)
    for u, v in ((a.mean, b.mean), (a.cov, b.cov), (c.mean, b.mean), (c.cov, b.cov)):
        np.testing.assert_array_equal(_bits64(u), _bits64(v))
    assert c.ranks is None
    # seeds drawn from rng: reproducible
    e = dfa.sbc_ranks(flow, xa, one, n_draws=N, rng=np.random.default_rng(3))
    f = dfa.sbc_ranks(flow, xa, one, n_draws=N, rng=np.random.default_rng(3))
    np.testing.assert_array_equal(e, f)
    hist = dfa.sbc_histogram(rk, N, 5)
    np.testing.assert_array_equal(hist, P.sbc_histogram(rk, N, 5))
    print(f"readme (untrained) rank histogram, dimension × 5 bins of 13:\n{hist}")


def test_posterior_stats_unconditional(cuda):
    flow = _flow("cfg2")
    d = flow.d
    x, _ = _inputs(d, 0, 40)
    h = flow.hip()
    r, blk, _ = _stats(h, cuda, x, np.zeros((0, 40), np.float32), 128, seed=5, offset=0, draws=False)
    st = dfa.posterior_stats(flow, n_draws=128, x=x, seed=5)
    assert st.mean.shape == (d, 40) and st.cov.shape == (d, d, 40)
    np.testing.assert_array_equal(st.ranks, r)
    np.testing.assert_array_equal(st.mean, P.moments(blk, d, 128)[0])
    np.testing.assert_array_equal(dfa.sbc_ranks(flow, x, n_draws=128, seed=5), r)
    s0 = dfa.posterior_stats(flow, n_draws=128, dims=(40,), seed=5)
    assert s0.ranks is None
    np.testing.assert_array_equal(_bits64(s0.cov), _bits64(st.cov))
