"""fp64 references of the weighted loss  loss_w = -Σ w_i·logpdf_i / Σ w_i  and its gradient.

numpy and the oracle only.  Both go through `O.nll_and_grad` as it stands:
  * integer weights k_i: the batch with column i repeated k_i times, mean over Σ k;
  * real weights: Σ w_i·g_i / W with g_i the gradient of sample i alone (n_total = 1), for
    small batches (one oracle pass per sample).
"""
import numpy as np

from oracle import flow_oracle as O
from train_edge_cases import _flat_oracle_grads


def duplicated(x, th, k):
    """(x, θ) with column i repeated k[i] times, in order."""
    idx = np.repeat(np.arange(x.shape[1]), np.asarray(k, dtype=np.int64))
    return np.ascontiguousarray(x[:, idx]), np.ascontiguousarray(th[:, idx])


def integer_weight_grad(spec, x, th, k):
    """(loss, flat gradient) for integer weights k (Σ k >= 1)."""
    xd, td = duplicated(x, th, k)
    loss, g = O.nll_and_grad(spec, xd, td, n_total=int(np.sum(k)))
    return float(loss), _flat_oracle_grads(spec, g)


def per_sample_grad(spec, x, th, w):
    """(loss, flat gradient) for real weights w: Σ w_i·(loss_i, g_i) / Σ w_i."""
    w = np.asarray(w, dtype=np.float64)
    W = float(np.sum(w))
    loss, grad = 0.0, None
    for i in range(x.shape[1]):
        li, gi = O.nll_and_grad(spec, x[:, i:i + 1], th[:, i:i + 1], n_total=1)
        gi = _flat_oracle_grads(spec, gi)
        grad = w[i] * gi if grad is None else grad + w[i] * gi
        loss += w[i] * float(li)
    return loss / W, grad / W
