"""Host reference of the histogram calls (df_hist.hip): np.histogram / np.histogram2d of the
same Float32 draws in the block layout of counts_out, and a brute-force loop over draws, tables
and bins that states the bin rule directly.

Bin rule: bin j (0 <= j < L) holds e_j <= v < e_{j+1}; the last bin also holds v == e_L; all
comparisons in Float32, −0 == +0; a draw below e_0, above e_L or NaN is counted nowhere in the
tables that keep that dimension; a 2-D table counts a draw when both coordinates are inside.
Block of a point: the tables in request order, table (a, b) at index i_a + L_a·i_b.
"""
import numpy as np


def corner(bins):
    """Every dimension with bins, then every pair of them: [(a,), ..., (a, b), ...]."""
    xs = [k for k in range(len(bins)) if bins[k] > 0]
    return [(a,) for a in xs] + [(a, b) for i, a in enumerate(xs) for b in xs[i + 1:]]


def sizes(keep, bins):
    return [int(bins[K[0]]) * (int(bins[K[1]]) if len(K) == 2 else 1) for K in keep]


def flat_edges(edges):
    """The edges of the dimensions that have some, one after the other, Float32."""
    return np.concatenate([np.asarray(e, np.float32) for e in edges if e is not None])


def bins_of(edges):
    return np.array([0 if e is None else len(e) - 1 for e in edges], np.int32)


def blocks(q, edges, keep):
    """(M, T) int32: the tables ``keep`` of every point of q (M, N, d) float32 with numpy.
    edges: d entries, a Float32 vector or None."""
    q = np.asarray(q)
    assert q.dtype == np.float32 and q.ndim == 3
    M = q.shape[0]
    bins = bins_of(edges)
    out = np.zeros((M, sum(sizes(keep, bins))), np.int32)
    for i in range(M):
        at = 0
        for K, size in zip(keep, sizes(keep, bins)):
            if len(K) == 1:
                h, _ = np.histogram(q[i, :, K[0]], np.asarray(edges[K[0]], np.float32))
                out[i, at:at + size] = h
            else:
                a, b = K
                h, _, _ = np.histogram2d(q[i, :, a], q[i, :, b],
                                         (np.asarray(edges[a], np.float32), np.asarray(edges[b], np.float32)))
                assert np.all(h == np.floor(h))
                out[i, at:at + size] = h.T.reshape(-1)                  # i_a + L_a · i_b
            at += size
    return out


def blocks_indexed(q, edges, keep):
    """blocks() for many tables (the corner at d = 32 and above, hundreds of points), where a
    numpy call per (point, table) takes minutes: the per-dimension bin indices as
    np.histogramdd finds them — np.searchsorted(edges, v, "right") − 1, the last edge moved into
    the last bin, everything else outside dropped — counted with np.bincount.  The host tests
    hold it equal to blocks()."""
    q = np.asarray(q)
    assert q.dtype == np.float32 and q.ndim == 3
    M, N, d = q.shape
    bins = bins_of(edges)
    idx = np.full((d, M, N), -1, np.int64)
    for k in range(d):
        if edges[k] is None:
            continue
        e = np.asarray(edges[k], np.float32)
        v = q[:, :, k]
        j = np.searchsorted(e, v, side="right") - 1
        j[v == e[-1]] = bins[k] - 1
        j[(j < 0) | (j >= bins[k])] = -1                                # also NaN: it sorts past every edge
        idx[k] = j
    out = np.zeros((M, sum(sizes(keep, bins))), np.int32)
    at = 0
    for K, size in zip(keep, sizes(keep, bins)):
        ia = idx[K[0]]
        ok = ia >= 0
        w = ia
        if len(K) == 2:
            ib = idx[K[1]]
            ok = ok & (ib >= 0)
            w = ia + int(bins[K[0]]) * ib
        flat = (np.arange(M)[:, None] * size + w)[ok]
        out[:, at:at + size] = np.bincount(flat, minlength=M * size).reshape(M, size)
        at += size
    return out


def bin_of(v, e):
    """The bin of one Float32 value under the rule above, or −1; a plain loop over the bins."""
    v = np.float32(v)
    L = len(e) - 1
    for j in range(L):
        if np.float32(e[j]) <= v and (v < np.float32(e[j + 1]) or (j == L - 1 and v == np.float32(e[L]))):
            return j
    return -1


def blocks_brute(q, edges, keep):
    """blocks() by the triple loop over points, draws and tables."""
    q = np.asarray(q)
    M, N, _ = q.shape
    bins = bins_of(edges)
    out = np.zeros((M, sum(sizes(keep, bins))), np.int32)
    for i in range(M):
        for j in range(N):
            at = 0
            for K, size in zip(keep, sizes(keep, bins)):
                ia = bin_of(q[i, j, K[0]], edges[K[0]])
                if len(K) == 1:
                    if ia >= 0:
                        out[i, at + ia] += 1
                else:
                    ib = bin_of(q[i, j, K[1]], edges[K[1]])
                    if ia >= 0 and ib >= 0:
                        out[i, at + ia + int(bins[K[0]]) * ib] += 1
                at += size
    return out


def ulp_neighbours(e):
    """One Float32 ulp below and above every value of e."""
    e = np.asarray(e, np.float32)
    return np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))


def plant(q, edges, rng):
    """Into every point of q (M, N, d), at random draws of every dimension with edges: each
    edge's own bits and its two ulp neighbours, NaN of both signs, ±inf, ±0 and values far
    outside — as many of them as the point has draws for.  In place."""
    M, N, d = q.shape
    nan = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
    for k in range(d):
        if edges[k] is None:
            continue
        e = np.asarray(edges[k], np.float32)
        lo, hi = ulp_neighbours(e)
        special = np.concatenate([e, lo, hi, nan, np.array([np.inf, -np.inf, 0.0, -0.0, 3e38, -3e38, 1e30, -1e30],
                                                           np.float32)])
        for i in range(M):
            take = rng.permutation(special)[:max(N // 2, 1)]
            rows = rng.permutation(N)[:take.size]
            q[i, rows, k] = take
    return q
