"""Reference of the marginal tables (df_flow_pdf_marginals, flows.pdf_marginals) in plain
numpy, float64 throughout, read-only.

A table of kept axes K over per-point values v (the pdf: exp of the fp64 oracle's
``g["lp"]`` of tests/grid_cases.py, or of the device's own ``logpdf_grid`` values cast to
fp64) is

    m_K[i_K] = Σ over the points p with kept indices i_K of  v[p] · ∏_{k ∉ K} w_k[i_k(p)]

A whole grid is reshaped to its lengths (``order="F"``: the first axis fastest), the weights of
the other axes applied and those axes summed; a window of a grid too large for that is
scattered point by point with the same index arithmetic as grid_cases.grid_points."""
import itertools

import numpy as np


def all_requests(na):
    """(), every single axis, every pair: the full request list of a grid of na axes."""
    return [()] + [(a,) for a in range(na)] + list(itertools.combinations(range(na), 2))


def table_shape(lens, keep):
    return tuple(int(lens[k]) for k in keep)


def marginal(values, lens, weights, keep, first=0):
    """The table of the kept axes ``keep`` (ascending) from the per-point values of points
    [first, first + len(values)) of the grid of lengths ``lens``; ``weights``: one float64
    vector per axis.  Shape (L_a,), (L_a, L_b) or ()."""
    lens = [int(L) for L in lens]
    na = len(lens)
    keep = tuple(keep)
    assert list(keep) == sorted(set(keep)) and all(0 <= k < na for k in keep)
    v = np.asarray(values, np.float64).reshape(-1)
    w = [np.asarray(x, np.float64) for x in weights]
    assert len(w) == na and all(x.shape == (L,) for x, L in zip(w, lens))
    P = int(np.prod(lens, dtype=object)) if lens else 1
    if first == 0 and v.size == P:
        t = v.reshape(lens, order="F")
        for k in range(na):
            if k not in keep:
                shape = [1] * na
                shape[k] = lens[k]
                t = t * w[k].reshape(shape)
        return t.sum(axis=tuple(k for k in range(na) if k not in keep))
    assert 0 <= first and first + v.size <= P < 2**62
    p = first + np.arange(v.size, dtype=np.int64)
    stride, idx = 1, []
    for L in lens:
        idx.append((p // stride) % L)
        stride *= L
    c = v.copy()
    for k in range(na):
        if k not in keep:
            c = c * w[k][idx[k]]
    out = np.zeros(table_shape(lens, keep), np.float64)
    if not keep:
        return out + c.sum()
    np.add.at(out, tuple(idx[k] for k in keep), c)
    return out


def marginals_of_logpdf(lp, lens, weights, keeps, first=0):
    """{keep: table} of exp(float64(lp)): ``lp`` the oracle's fp64 values or the device's fp32."""
    v = np.exp(np.asarray(lp).astype(np.float64))
    return {tuple(K): marginal(v, lens, weights, K, first) for K in keeps}


def terms_per_bin(lens, keep, count=None):
    """Points that fall into one bin of a whole grid (an upper bound for a window of
    ``count`` points)."""
    n = 1
    for k, L in enumerate(lens):
        if k not in keep:
            n *= int(L)
    return n if count is None else min(n, count)
