"""Host reference of the order-statistics calls (df_quant.hip): the totalOrder key of a Float32
and its inverse, the order statistics of per-point draws by a sort of the keys, and the two-order
interpolation behind a quantile."""
import numpy as np

U = 2.0 ** -52


def keys(v):
    """uint32 keys of float32 values: bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000).  Compared as
    unsigned integers they give IEEE totalOrder: −NaN < −inf < ... < −0 < +0 < ... < +inf < +NaN."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def values(k):
    """The float32 values of keys: the inverse of :func:`keys`, bit for bit."""
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> np.uint32(31) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def order_stats(draws, orders):
    """out[i, k, q] = the draw of point i's dimension k whose key is the orders[q]-th smallest,
    for float32 draws (M, N, d) → float32 (M, d, Q), with the draw's own bits."""
    q = np.asarray(draws)
    assert q.dtype == np.float32 and q.ndim == 3
    o = np.asarray(orders, np.int64).reshape(-1)
    assert o.size and o.min() >= 0 and o.max() < q.shape[1]
    s = np.sort(keys(q).reshape(q.shape), axis=1)              # (M, N, d)
    return np.ascontiguousarray(values(s[:, o, :]).reshape(q.shape[0], o.size, q.shape[2]).transpose(0, 2, 1))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def linear_orders(p, N):
    """(j, hi, g) of the linear (type 7) rule: h = p·(N − 1), j = floor(h), hi = min(j + 1, N − 1),
    g = h − j."""
    h = float(p) * (N - 1)
    j = min(int(np.floor(h)), N - 1)
    return j, min(j + 1, N - 1), h - j


def interpolate(lo, hi, g):
    """lo + (hi − lo)·g in float64."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return lo + (hi - lo) * g


def interp_bound(lo, hi):
    """What two evaluations of the linear rule in float64 may differ by: 4·2^-52·max(|lo|, |hi|)
    (a subtraction, a product and a sum, each rounded once, in either of the two usual forms)."""
    return 4 * U * np.maximum(np.abs(np.asarray(lo, np.float64)), np.abs(np.asarray(hi, np.float64)))


def quantiles(draws, probs):
    """(value, bound), both (P, d, M) float64: the linear quantiles of float32 draws (M, N, d) from
    two order statistics each, and interp_bound of the two."""
    q = np.asarray(draws)
    N = q.shape[1]
    val, bnd = [], []
    for p in probs:
        j, hi, g = linear_orders(p, N)
        os_ = order_stats(q, [j, hi]).astype(np.float64)        # (M, d, 2)
        val.append(interpolate(os_[:, :, 0], os_[:, :, 1], g).T)
        bnd.append(interp_bound(os_[:, :, 0], os_[:, :, 1]).T)
    return np.stack(val), np.stack(bnd)
