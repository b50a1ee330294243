"""The SPLIT kernels' activation split forms its remainders c - hi on the matrix pipe
(df::uni::mrem, densityflows.jl_amd/csrc/df_uniform_impl.h).  Two properties that hold
whichever matrix instruction and schedule do that work:

1. a non-finite sample stays local: the remainder instruction multiplies by zeros, and
   0 * inf = NaN must not reach another sample (the 4x4x4 form shares a 4x4 block among
   the four lanes of samples 4..7; the 16x16x16 form shares one among 16 samples);
2. the outputs are the pinned bits of tests/golden/split_pin_*.npy
   (tests/golden/make_split_pin.py states the commit they come from)."""
import numpy as np
import pytest

import make_split_pin as P


@pytest.fixture(scope="module")
def cfg2(cuda):
    import bench

    hc = bench.build_chain("cfg2").hip(device=0, n_hint=0)
    assert hc.info.kernel == 4, hc.info.kernel
    return hc


def _passes(hc, z, cuda):
    """forward of z, then inverse and per-sample logpdf of that x: six arrays."""
    import torch

    B = z.size // P.D
    tz = torch.from_numpy(z).to(cuda)
    x, ldj = torch.empty_like(tz), torch.empty(B, device=cuda)
    hc.run("forward", tz, None, x, ldj, B)
    zb, ldjb, lp = torch.empty_like(tz), torch.empty(B, device=cuda), torch.empty(B, device=cuda)
    # the inverse and logpdf passes get the same poisoned sample as their input
    hc.run("backward", tz, None, zb, ldjb, B)
    hc.run_logpdf(tz, None, lp, B)
    torch.cuda.synchronize()
    return {"fwd_x": x.cpu().numpy().reshape(B, P.D), "fwd_ldj": ldj.cpu().numpy(),
            "inv_x": zb.cpu().numpy().reshape(B, P.D), "inv_ldj": ldjb.cpu().numpy(), "logpdf": lp.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), 3e38])
def test_nonfinite_sample_stays_local(cuda, cfg2, bad):
    B, smp = 48, 5  # one full two-tile group plus a half group; sample 5 shares a 4x4 block with 4, 6, 7
    z = np.random.default_rng(5).standard_normal((B, P.D)).astype(np.float32)
    clean = _passes(cfg2, z.reshape(-1).copy(), cuda)
    others = np.arange(B) != smp
    for dim in (0, P.D - 1):  # a conditioner feature of the first layer / of the second
        zp = z.copy()
        zp[smp, dim] = bad
        dirty = _passes(cfg2, zp.reshape(-1), cuda)
        if np.isnan(bad):
            assert not np.all(np.isfinite(dirty["fwd_x"][smp])), "the poisoned sample itself came out finite"
        for k, v in clean.items():
            assert np.all(np.isfinite(v[others])), k
            a, b = v[others], dirty[k][others]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, dim, np.argwhere(a != b)[:4])


@pytest.mark.gpu
def test_pinned_bits(cuda):
    want = {k: np.load(P.path(k)) for k in P.NAMES}
    got = P.compute(fwd_x=want["fwd_x"])
    for k in P.NAMES:
        print(k, want[k].shape, "differing:", int(np.sum(want[k].view(np.uint32) != got[k].view(np.uint32))))
    for k in P.NAMES:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
