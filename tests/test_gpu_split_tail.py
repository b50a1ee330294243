"""The tail of a net body of the specialised SPLIT kernel (densityflows.jl_amd/csrc/
df_uniform_impl.h, net_tiles' read-ahead path): the transposed reduction of the output
GEMV, the coupling, the ldj update and the first-Dense split may be re-arranged, the
arithmetic, its order and its roundings may not.  So every pass (forward, forward!,
inverse, per-sample logpdf, the fp64 NLL partial sum) on every model of
tests/golden/make_tail_pin.py gives the pinned bits of tests/golden/tail_pin_*.npz (the
generator states the commit they come from), at DF_TILES = 2, 4 and the plan's maximum, at
batches 1, 17, S - 1, S, S + 1 and 2S + 33 (S = 128 · tiles), and the launches ran the
specialised SPLIT kernel with that many tiles per wave."""
import numpy as np
import pytest

import make_tail_pin as P

pytestmark = pytest.mark.gpu

META = P.meta()


def _cases():
    return [(name, t) for name in sorted(P.MODELS) for t in P.tile_settings(META["max_tiles"][name])]


@pytest.mark.parametrize("name,tiles", _cases())
def test_pinned_bits(cuda, monkeypatch, name, tiles):
    assert META["commit"].startswith(P.PARENT) and META["full_max"] == P.FULL_MAX
    want = np.load(P.path(name))
    monkeypatch.setenv("DF_DEBUG_LAUNCH", "1")
    monkeypatch.setenv("DF_TILES", str(tiles))
    hc = P.compile_model(name)
    assert hc.info.kernel == 4, hc.info.kernel
    bad = []
    for B in P.batches(tiles):
        got, ran = P.launch_lines(lambda: P.passes(hc, name, B))
        assert len(ran) >= 4, ran
        for _, batch, kernel, t, max_t in ran:
            assert kernel == "uniform-fast-split" and int(batch) == B, ran
            assert int(t) == tiles, f"{name} DF_TILES={tiles}: batch {batch} ran {t} tiles per wave"
            assert int(max_t) == META["max_tiles"][name], (name, max_t)
        for k in P.PASSES + ("fwdi_x", "nll"):
            key = f"nll_t{tiles}_{B}" if k == "nll" else f"{'fwd_x' if k == 'fwdi_x' else k}_{B}"
            w = want[key]
            g = got[k] if k == "nll" else P.pinned(got[k], B)
            assert g.shape == w.shape and g.dtype == w.dtype, (k, B)
            n = int(np.sum(g.view(np.uint8) != w.view(np.uint8)))
            if n:
                bad.append((k, B, n))
    assert not bad, f"(pass, batch, differing bytes of the array or of its SHA-256): {bad}"
