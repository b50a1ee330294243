"""numpy restatement of df_flow_sample_region's contract (include/densityflows_hip.h): the
Float32 predicate of a region, operation for operation, and the ordered selection of the
first n_want accepted candidates.  Pinned on literals in tests/test_reject_host.py; the GPU
tests build every expectation with it from candidates that HIPChain.run_sample returns."""
import numpy as np

F = np.float32


def predicate(x, lo=None, hi=None, A=None, b=None):
    """x (d, N) Float32 → bool (N,).  Box: lo[k] <= x[k] <= hi[k] as written (a NaN coordinate
    rejects).  Half-space h: acc = A[h,0]*x[0]; acc = acc + A[h,k]*x[k], k = 1..d-1, each
    product and each sum rounded to Float32; acc <= b[h]."""
    x = np.asarray(x, F)
    d, N = x.shape
    ok = np.ones(N, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if lo is not None:
            ok &= np.all(np.broadcast_to(np.asarray(lo, F), (d,))[:, None] <= x, axis=0)
        if hi is not None:
            ok &= np.all(x <= np.broadcast_to(np.asarray(hi, F), (d,))[:, None], axis=0)
        if A is not None:
            A = np.asarray(A, F).reshape(-1, d)
            b = np.asarray(b, F).reshape(-1)
            for h in range(A.shape[0]):
                acc = (A[h, 0] * x[0]).astype(F)
                for k in range(1, d):
                    acc = (acc + (A[h, k] * x[k]).astype(F)).astype(F)
                ok &= acc <= b[h]
    return ok


def first_accepted(cands, mask, n_want, max_tries):
    """cands (d, N), mask (N,) → (rows (d, accepted), tried, accepted): the first n_want
    candidates with mask set among those of index < max_tries, in order; tried = 1 + the
    index of the one that filled the last slot, else the number examined, min(N, max_tries)."""
    cands = np.asarray(cands)
    mask = np.asarray(mask, bool)
    examined = min(mask.shape[0], max_tries)
    idx = np.flatnonzero(mask[:examined])[:n_want]
    accepted = idx.shape[0]
    tried = int(idx[-1]) + 1 if accepted == n_want and n_want > 0 else examined
    return cands[:, idx].copy(), tried, accepted
