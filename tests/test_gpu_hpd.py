"""GPU tests of the calibration call (df_calib.hip): df_flow_hpd_ranks and its Python mirror
hpd_levels / expected_coverage.

Chains: those of tests/test_gpu_moments.py::_chain — "readme" (n = 1), "cfg2" (n = 0), "wide"
(n = 3, layer-wise class, hidden 256) — with θ bounds (−1, 3) and points from _inputs.

Kernel families.  Every batch here — the points (at most 257) and the draws of a call or of
one chunk (at most 2 · 4100 = 8200 samples) — lies below the README-class chain's small-kernel
crossover (16 · 8 · CUs samples, 32768 on 256 CUs), and cfg2 and wide have one chain-pass
kernel family at any size.  So every bitwise comparison below stays inside one family; no test
compares across families.

No test states a statistical claim: the model is untrained.  The coverage curve is printed.
"""
import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd.data import MetaData
from helpers import close, spec_to_element
import hpd_ref as H
from test_gpu_moments import _bounds, _chain
from test_gpu_score import _spec
from test_gpu_train import _dev, _inputs

pytestmark = pytest.mark.gpu

GUARD = 8
INT32_MIN = -(2 ** 31)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ranks(h, cuda, x, th, N, chunk=0, seed=77, offset=3, lp=True, draws=True, shift=0, M=None):
    """One df_flow_hpd_ranks call on numpy x (d, M), θ (n, M) → (ranks, lp or None, draws
    (M, N) or None).  Every output is followed by GUARD elements (INT32_MIN, NaN) that must
    survive; ``shift``: the draws' buffer starts that many floats past a 16-byte boundary."""
    import torch

    M = x.shape[1] if M is None else M
    n = th.shape[0]
    rank = torch.full((M + GUARD,), INT32_MIN, dtype=torch.int32, device=cuda)
    lpb = torch.full((M + GUARD,), np.nan, dtype=torch.float32, device=cuda) if lp else None
    dbuf = torch.full((4 + M * N + GUARD,), np.nan, dtype=torch.float32, device=cuda) if draws else None
    nan_bits = _bits(np.float32(np.nan).reshape(1))[0]
    h.run_hpd_ranks(_dev(x, cuda) if M else None, _dev(th, cuda) if n and M else None, M, N, chunk, seed, offset,
                    rank, lpb, dbuf[shift:] if draws else None)
    torch.cuda.synchronize()
    r = rank.cpu().numpy()
    assert np.all(r[M:] == INT32_MIN), "rank_out written past n_points"
    out = [r[:M].copy(), None, None]
    if lp:
        v = lpb.cpu().numpy()
        assert np.all(_bits(v[M:]) == nan_bits), "logpdf_out written past n_points"
        out[1] = v[:M].copy()
    if draws:
        v = dbuf.cpu().numpy()
        assert np.all(_bits(v[:shift]) == nan_bits) and np.all(_bits(v[shift + M * N:]) == nan_bits), \
            "draws_logpdf_out written outside n_points · n_draws"
        out[2] = v[shift:shift + M * N].reshape(M, N).copy()
    return tuple(out)


# ---------------------------------------------------------------------------
# 1. counts are exact
# ---------------------------------------------------------------------------

# L = N / 4 lanes per point.  (1, 4), (3, 12), (17, 64), (5, 68), (257, 4): several points per
# wave (L = 1, 3, 16, 17), group edges inside a wave, a last wave partly filled, 257 points past
# one workgroup of 4 · 64 points.  (3, 260): a wave per point, the second trip one lane.
# (2, 4100): a workgroup per point, 5 trips of 256 lanes, the last one lane.
SHAPES = [(1, 4), (3, 12), (17, 64), (5, 68), (3, 260), (257, 4), (2, 4100)]


@pytest.mark.parametrize("name", ["readme", "cfg2", "wide"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_counts_are_exact(cuda, name, M, N):
    spec, d, n, h = _chain(name)
    x, th = _inputs(d, n, M)
    r, lp, q = _ranks(h, cuda, x, th, N)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(q)), "outputs not fully overwritten"
    np.testing.assert_array_equal(r, H.ranks(lp, q))
    assert r.dtype == np.int32 and np.all((0 <= r) & (r <= N))
    # the other template instance: no store of the draws' lp
    r2, lp2, _ = _ranks(h, cuda, x, th, N, draws=False)
    np.testing.assert_array_equal(r2, r)
    np.testing.assert_array_equal(_bits(lp2), _bits(lp))
    # the points' lp in the chain's workspace
    r3, _, _ = _ranks(h, cuda, x, th, N, lp=False, draws=False)
    np.testing.assert_array_equal(r3, r)
    # a draws buffer off the 16-byte boundary: scalar stores, the same values
    r4, _, q4 = _ranks(h, cuda, x, th, N, shift=1)
    np.testing.assert_array_equal(r4, r)
    np.testing.assert_array_equal(_bits(q4), _bits(q))
    print(f"{name} M={M} N={N}: ranks {r[:8]}")


# ---------------------------------------------------------------------------
# 2. the draws are the documented ones
# ---------------------------------------------------------------------------

# batches: 17 points; 17 · 68 = 1156 draws in one chunk and in the df_flow_sample_logpdf call
@pytest.mark.parametrize("name", ["readme", "cfg2", "wide"])
def test_draws_are_sample_logpdf(cuda, name):
    import torch

    spec, d, n, h = _chain(name)
    M, N, seed, offset = 17, 68, 4321, 6
    x, th = _inputs(d, n, M)
    r, lp, q = _ranks(h, cuda, x, th, N, seed=seed, offset=offset)
    xs = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    lps = torch.full((M * N,), np.nan, dtype=torch.float32, device=cuda)
    h.run_sample_logpdf(xs, lps, _dev(np.repeat(th, N, axis=1), cuda) if n else None, False, M * N, seed, offset)
    back = torch.full((M,), np.nan, dtype=torch.float32, device=cuda)
    h.run_logpdf(_dev(x, cuda), _dev(th, cuda) if n else None, back, M)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(q.ravel()), _bits(lps.cpu().numpy()))
    np.testing.assert_array_equal(_bits(lp), _bits(back.cpu().numpy()))


# ---------------------------------------------------------------------------
# 3. parity with the fp64 oracle
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["readme", "cfg2", "wide"])
def test_ranks_against_oracle(cuda, name):
    """The cap Σ(hi − lo) <= 0.01 · M · N is a property of the lp distribution, not of the
    Philox stream: tests/test_hpd_host.py::test_bracket_is_tight_for_the_oracle_alone holds the
    oracle alone to it on the CPU, with numpy normal draws, for these chains, points, θ and
    (M, N).  Observed share Σ(hi − lo) / (M · N) there: readme 0.00023, cfg2 0.00045, wide 0.00023
    (one or two draws of 4420 undecided)."""
    import torch

    spec, d, n, h = _chain(name)
    M, N, seed, offset = H.ORACLE_M, H.ORACLE_N, 2025, 1
    x, th = _inputs(d, n, M)
    r, lp, q = _ranks(h, cuda, x, th, N, seed=seed, offset=offset)
    z = torch.empty(d * M * N, dtype=torch.float32, device=cuda)
    h.random_normal(z, d * M * N, seed, offset)
    torch.cuda.synchronize()
    z64 = z.cpu().numpy().reshape(M * N, d).T.astype(np.float64)
    lp_p, lp_q = H.oracle_lp(spec, x, th, z64, N, *_bounds(n))
    ok, rp = close(lp, lp_p)
    assert ok, rp
    ok, rq = close(q, lp_q)
    assert ok, rq
    lo, hi = H.bracket(lp_p, lp_q)
    print(f"{name}: parity ratios points {rp:.3f} draws {rq:.3f}; bracket share "
          f"{np.sum(hi - lo) / (M * N):.5f}; ranks {r[:8]}")
    assert np.all(lo <= r) and np.all(r <= hi), (lo, r, hi)
    assert np.sum(hi - lo) <= 0.01 * M * N


# ---------------------------------------------------------------------------
# 4. independence of chunking and of the other points
# ---------------------------------------------------------------------------

# M = 7, N = 260: chunk 0 and 2^14 take the 1820 draws at once, 520 two points at a time (the
# last chunk one point), 260 and 100 (below N) one point at a time: batches of 260 .. 1820
# samples, all in one kernel family (see the module docstring).
@pytest.mark.parametrize("name", ["readme", "cfg2"])
def test_chunking_and_other_points(cuda, name):
    spec, d, n, h = _chain(name)
    M, N, seed, offset = 7, 260, 11, 4
    x, th = _inputs(d, n, M)
    r, lp, q = _ranks(h, cuda, x, th, N, seed=seed, offset=offset)
    for chunk in (260, 520, 100, 1 << 14):
        rc, lpc, qc = _ranks(h, cuda, x, th, N, chunk=chunk, seed=seed, offset=offset)
        np.testing.assert_array_equal(rc, r, err_msg=f"chunk {chunk}")
        np.testing.assert_array_equal(_bits(lpc), _bits(lp))
        np.testing.assert_array_equal(_bits(qc), _bits(q))
        rn, _, _ = _ranks(h, cuda, x, th, N, chunk=chunk, seed=seed, offset=offset, lp=False, draws=False)
        np.testing.assert_array_equal(rn, r, err_msg=f"chunk {chunk}, ranks alone")
    # point 3 alone, at its own counter
    r3, lp3, q3 = _ranks(h, cuda, x[:, 3:4], th[:, 3:4], N, seed=seed, offset=offset + d * 3 * N // 4)
    assert r3[0] == r[3]
    np.testing.assert_array_equal(_bits(q3[0]), _bits(q[3]))
    np.testing.assert_array_equal(_bits(lp3), _bits(lp[3:4]))


# ---------------------------------------------------------------------------
# 5. special values
# ---------------------------------------------------------------------------

def test_special_values(cuda):
    spec, d, n, h = _chain("readme")
    M, N = 5, 260
    x, th = _inputs(d, n, M)
    r, lp, q = _ranks(h, cuda, x, th, N)
    bad = x.copy()
    bad[:, 1] = np.nan
    bad[0, 3] = 1e30
    rb, lpb, qb = _ranks(h, cuda, bad, th, N)
    assert np.isnan(lpb[1]) and rb[1] == 0
    assert not np.isfinite(lpb[3]) or lpb[3] <= np.min(qb[3])
    with np.errstate(invalid="ignore"):
        assert rb[3] == np.sum(qb[3] > lpb[3])
    print(f"far point: lp = {lpb[3]}, rank {rb[3]} of {N}; NaN point: lp = {lpb[1]}, rank {rb[1]}")
    np.testing.assert_array_equal(rb, H.ranks(lpb, qb))
    # the draws do not depend on the points; the other points are unchanged
    np.testing.assert_array_equal(_bits(qb), _bits(q))
    keep = [0, 2, 4]
    np.testing.assert_array_equal(rb[keep], r[keep])
    np.testing.assert_array_equal(_bits(lpb[keep]), _bits(lp[keep]))
    # without the stored lp the same ranks
    rn, _, _ = _ranks(h, cuda, bad, th, N, lp=False, draws=False)
    np.testing.assert_array_equal(rn, rb)


def test_empty_call_writes_nothing(cuda):
    spec, d, n, h = _chain("readme")
    x, th = _inputs(d, n, 0)
    r, lp, q = _ranks(h, cuda, x, th, 8, M=0)       # the guards (every element) are checked inside
    assert r.shape == (0,) and lp.shape == (0,) and q.shape == (0, 8)


# ---------------------------------------------------------------------------
# 6. Python
# ---------------------------------------------------------------------------

def _flow(name):
    spec, d, n = _spec(name)
    return dfa.Flow(spec_to_element(spec), metadata=MetaData("", d, n, *_bounds(n)))


def test_hpd_levels(cuda):
    import torch

    flow = _flow("readme")
    d, n, dims, N, seed = 5, 1, (3, 5), 64, 19
    x, th = _inputs(d, n, 15)
    h = flow.hip()
    # the low-level call on the flat (Julia-order) points
    r, lp, _ = _ranks(h, cuda, x, th, N, seed=seed, offset=0)
    xa = np.asfortranarray(x).reshape((d,) + dims, order="F")
    tha = np.asfortranarray(th).reshape((n,) + dims, order="F")
    lv, rk, lpp = dfa.hpd_levels(flow, xa, tha, n_draws=N, seed=seed, return_ranks=True, return_logpdf=True)
    assert lv.shape == dims and lv.dtype == np.float64
    assert rk.shape == dims and rk.dtype == np.int32 and lpp.shape == dims and lpp.dtype == np.float32
    np.testing.assert_array_equal(rk.ravel(order="F"), r)
    np.testing.assert_array_equal(lv, rk / N)
    np.testing.assert_array_equal(_bits(lpp.ravel(order="F")), _bits(lp))
    # device tensors in, the same levels; levels alone
    xt = torch.from_numpy(np.ascontiguousarray(xa)).to(cuda)
    tht = torch.from_numpy(np.ascontiguousarray(tha)).to(cuda)
    lv2 = dfa.hpd_levels(flow, xt, tht, n_draws=N, seed=seed, chunk=128)
    assert isinstance(lv2, np.ndarray)
    np.testing.assert_array_equal(lv2, lv)
    # an NTuple θ is that θ in every column
    one = (1.25,)
    lv3, rk3 = dfa.hpd_levels(flow, xa, one, n_draws=N, seed=seed, return_ranks=True)
    r3, _, _ = _ranks(h, cuda, x, np.full((n, 15), 1.25, np.float32), N, seed=seed, offset=0)
    np.testing.assert_array_equal(rk3.ravel(order="F"), r3)
    np.testing.assert_array_equal(lv3, rk3 / N)
    # seeds drawn from rng: reproducible
    a = dfa.hpd_levels(flow, xa, one, n_draws=N, rng=np.random.default_rng(3))
    b = dfa.hpd_levels(flow, xa, one, n_draws=N, rng=np.random.default_rng(3))
    np.testing.assert_array_equal(a, b)
    c, cov = dfa.expected_coverage(lv)
    np.testing.assert_array_equal(cov, H.expected_coverage(lv)[1])
    print("readme (untrained) coverage at c = 0, 0.1, ..., 1:", np.round(cov[::10], 3))


def test_hpd_levels_unconditional(cuda):
    flow = _flow("cfg2")
    d = flow.d
    x, _ = _inputs(d, 0, 40)
    lv, rk = dfa.hpd_levels(flow, x, n_draws=128, seed=5, return_ranks=True)
    assert lv.shape == (40,) and rk.shape == (40,)
    h = flow.hip()
    r, _, _ = _ranks(h, cuda, x, np.zeros((0, 40), np.float32), 128, seed=5, offset=0)
    np.testing.assert_array_equal(rk, r)
    c, cov = dfa.expected_coverage(lv)
    assert c.shape == cov.shape == (101,) and cov[-1] == 1.0
    print("cfg2 (untrained) coverage at c = 0, 0.1, ..., 1:", np.round(cov[::10], 3))
