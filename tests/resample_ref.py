"""Host reference of df_draw_resample in pure integers: Philox4x32-10 on numpy uint64 words, the
quantised weights, their scan and the picks in Python ``int`` (the 112-bit products never round).
Nothing here comes from the library.

    q_j  = rint(ldexp(w_j, 32 − e)) for finite w_j > 0, else 0; wmax = f·2^e, f in [0.5, 1)
    C    = the exclusive scan of q, T = C_N
    pick = the j with C_j·D <= num·T < C_{j+1}·D, found as floor(num·T / D) located in C
"""
import numpy as np

SYSTEMATIC, STRATIFIED, MULTINOMIAL = 0, 1, 2
METHODS = {"systematic": SYSTEMATIC, "stratified": STRATIFIED, "multinomial": MULTINOMIAL}

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """``counter`` (..., 4) and ``key`` (2,) of 32-bit words → the (..., 4) output words (uint64
    arrays holding 32-bit values)."""
    c = np.asarray(counter, dtype=np.uint64) & _LOW
    c0, c1, c2, c3 = (c[..., e].copy() for e in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 × 32 bits: exact in 64
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LOW)
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1)


def _words(seed, ctr):
    """The four output words of every 64-bit counter value in ``ctr`` (Python ints, any size: taken
    mod 2^64) on the resampler's stream: counter (low, high, 1, 0), key (seed low, seed high)."""
    c = np.array([[v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF, 1, 0] for v in ctr], dtype=np.uint64).reshape(-1, 4)
    return philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def quantise(w):
    """One point's Float32 weights → the list of its q_j as Python ints."""
    w = np.asarray(w, dtype=np.float32).ravel()
    with np.errstate(invalid="ignore"):
        part = np.isfinite(w) & (w > 0)
    if not part.any():
        return [0] * w.size
    w64 = np.where(part, w, np.float32(0)).astype(np.float64)
    _, e = np.frexp(w64.max())
    q = np.rint(np.ldexp(w64, 32 - int(e)))              # exact scale, round half to even
    return [int(v) for v in q]


def scan(q):
    """C_0 .. C_N of the q_j."""
    c = [0]
    for v in q:
        c.append(c[-1] + v)
    return c


def numerators(M, K, method, seed, offset):
    """(num (M, K) as Python ints in an object array, D)."""
    num = np.empty((M, K), dtype=object)
    ks = np.arange(K)
    if method == SYSTEMATIC:
        r = _words(seed, [offset + i for i in range(M)])[:, 0]
        for i in range(M):
            num[i] = [(k << 32) + int(r[i]) for k in range(K)]
        return num, K << 32
    if method == STRATIFIED:
        for i in range(M):
            wd = _words(seed, [offset + i * (K // 4) + c for c in range(K // 4)])
            r = wd[ks // 4, ks % 4]
            num[i] = [(k << 32) + int(r[k]) for k in range(K)]
        return num, K << 32
    assert method == MULTINOMIAL
    for i in range(M):
        wd = _words(seed, [offset + i * (K // 2) + c for c in range(K // 2)])
        lo, hi = wd[ks // 2, 2 * (ks % 2)], wd[ks // 2, 2 * (ks % 2) + 1]
        num[i] = [(int(hi[k]) << 32) + int(lo[k]) for k in range(K)]
    return num, 1 << 64


def locate(c, v):
    """The j with c[j] <= v < c[j + 1] for every v (Python ints below c[-1] < 2^56)."""
    return np.searchsorted(np.array(c[1:], dtype=np.uint64), np.array(v, dtype=np.uint64), side="right")


def picks(w, K, method, seed, offset=0):
    """``w`` (M, N) Float32 → the (M, K) int32 picks of df_draw_resample; ``method`` a code or a name."""
    method = METHODS.get(method, method)
    w = np.asarray(w, dtype=np.float32)
    M, N = w.shape
    num, D = numerators(M, K, method, int(seed), int(offset))
    out = np.full((M, K), -1, dtype=np.int32)
    for i in range(M):
        c = scan(quantise(w[i]))
        T = c[-1]
        if T == 0:
            continue
        assert T < 1 << 56
        out[i] = locate(c, [n * T // D for n in num[i]])
    return out


def gather(draws, idx):
    """``draws`` (M, N, d) Float32 and picks (M, K) → the picked rows (M, K, d), all-NaN (0x7fc00000)
    where the pick is −1."""
    draws = np.asarray(draws, dtype=np.float32)
    M, K = idx.shape
    out = np.take_along_axis(draws, np.maximum(idx, 0)[:, :, None].astype(np.int64), axis=1)
    out.view(np.uint32)[idx < 0] = 0x7fc00000
    return out
