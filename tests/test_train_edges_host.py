"""CPU side of the training edge matrix: what the matrix's value check is worth.

tests/test_gpu_train_edges.py compares gradients of batches that make every training
kernel take a second and third trip through its batch loop with the fp64 oracle.  That
only guards those loops if a lost trip fails the criterion.  The smallest loss a loop
fault can cause is one 16-sample tile; here the oracle itself leaves the last tile of the
batch out (keeping the full batch's 1/B) and is held against the full gradient under the
GPU test's criterion, helpers.close(g, ref, 1e-4, 2e-5) per Dense tensor.  The worst
per-tensor violation ratio must be at least 4, at every batch the GPU test can have as a
case's largest (train_edge_cases.largest_batches: by the fused kernel's occupancy).

Measured with the oracle (worst ratio over the Dense tensors / the smallest tensor's):

    chain         B = 821      1025       1553       1589
    readme       179 / 13   129 / 14    89 / 9.1   99 / 6.5
    cfg2         488 / 2.6  292 / 3.5  185 / 2.0  364 / 2.6
    mixed        363 / 29   378 / 18   383 / 21   470 / 20
    pre          178 / 1.2  133 / 3.4   86 / 2.0  112 / 2.6
    wide                                           88 / 2.8
    cfg5x2                                        272 / 5.3
    cfg5_in52                                     253 / 4.8

(pre: the softplus / swish / logcosh chain; cfg5_in52: the 52-input first Dense.)
"""
import numpy as np
import pytest

import train_edge_cases as T
from helpers import close

MIN_RATIO = 4.0


def _params():
    seen, out = set(), []
    for chain, _, form, _ in T.CASES.values():
        for B in T.largest_batches(form):
            if (chain, B) not in seen:
                seen.add((chain, B))
                out.append((chain, B))
    return out


def test_batches_of_the_matrix():
    """The lists the issue of this matrix gives for one workgroup per CU at two CUs."""
    assert T.batches(T.fused_trips(2)) == [255, 256, 257, 529, 821]
    assert T.batches(T.layerwise_trips(2), T.LAYERWISE_EXTRA) == [255, 256, 257, 511, 512, 513, 529, 821, 1041, 1553,
                                                                   1589]
    assert T.batches(T.score_trips(8)) == [511, 512, 513, 1041, 1589]
    for form in ("FUSED", "KEPT"):
        assert all(b < T.B_LIMIT for b in T.largest_batches(form))
    # every case names a chain, and the chains of one case family share their oracle
    assert all(c[0] in T.EDGE_SPECS for c in T.CASES.values())


@pytest.mark.parametrize("chain,B", _params())
def test_lost_tile_fails_the_value_check(chain, B):
    spec = T.case_data(chain)[0]
    _, full = T.oracle_grad(chain, B)
    _, part = T.oracle_grad(chain, B, drop_last_tile=True)
    ratios = [close(part[sl], full[sl], T.G_RTOL, T.G_ATOL)[1] for sl in T._tensor_slices(spec)]
    print(f"LOST-TILE {chain} B={B}: worst ratio {max(ratios):.1f}, smallest {min(ratios):.2f}")
    assert np.all(np.isfinite(full)) and full.shape == part.shape
    assert max(ratios) >= MIN_RATIO, f"{chain} B={B}: a lost tile moves the gradient by only {max(ratios):.2f} tolerances"
