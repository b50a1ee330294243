"""Pair trees of the specialised SPLIT kernel's net-body tail (densityflows.jl_amd/csrc/
df_uniform_impl.h, net_tiles' read-ahead path): a net of three or four outputs reduces both
tiles of a tile group in one pair of trees, the s outputs of both tiles are summed in one
tree and both rows' ldj words are updated once.  The arithmetic, its order and its roundings
stay, so every pass (forward, forward!, inverse, per-sample logpdf, the fp64 NLL partial
sum) on every model of tests/golden/make_pair_tree_pin.py gives the pinned bits of
tests/golden/pair_tree_pin_*.npz (the generator states the commit they come from), at
DF_TILES = 2 and 4 (4 where the model's plan has room for four tiles per wave: d = 6 and 7 at
hidden 64 stop at 2), at batches 1, 15, 16, 17, 31, 32, 33, S + 1 and S + 17 (S = 128 · tiles;
at S + 17 the second tile of the last pair is wholly past the batch end), and every launch
ran the kernel the pins were taken on with that many tiles per wave.

The specialised kernel takes at most three conditioner inputs, so the d = 7 chain of a
three- and a four-output layer and the d = 8 chain select another kernel (the generator's
note); they are pinned as well, and d6 (3 | 3 | 3) and d7q (4 | 4 | 4) reach the three- and
four-output bodies of the specialised kernel in their place."""
import numpy as np
import pytest

import make_pair_tree_pin as P
import make_tail_pin as T

pytestmark = pytest.mark.gpu

META = P.meta()


def _cases():
    return [(name, t) for name in sorted(P.MODELS) for t in P.tile_settings(name, META["max_tiles"])]


@pytest.mark.parametrize("name,tiles", _cases())
def test_pinned_bits(cuda, monkeypatch, name, tiles):
    assert META["commit"].startswith(P.PARENT) and META["full_max"] == P.FULL_MAX
    want = np.load(P.path(name))
    monkeypatch.setenv("DF_DEBUG_LAUNCH", "1")
    monkeypatch.setenv("DF_TILES", str(tiles))
    hc = P.compile_model(name)
    bad = []
    for B in P.batches(tiles):
        got, ran = T.launch_lines(lambda: P.passes(hc, name, B))
        assert all(int(batch) == B for _, batch, _, _, _ in ran), ran
        assert P.launches(ran) == META["kernels"][f"{name}_t{tiles}_{B}"], (name, tiles, B, ran)
        if P.MODELS[name][4]:
            assert len(ran) >= 4 and all(k == "uniform-fast-split" and t == tiles for k, t in P.launches(ran)), ran
        for k in P.PASSES + ("fwdi_x", "nll"):
            key = f"nll_t{tiles}_{B}" if k == "nll" else f"{'fwd_x' if k == 'fwdi_x' else k}_{B}"
            w = want[key]
            g = got[k] if k == "nll" else P.pinned(got[k], B)
            assert g.shape == w.shape and g.dtype == w.dtype, (k, B)
            n = int(np.sum(g.view(np.uint8) != w.view(np.uint8)))
            if n:
                bad.append((k, B, n))
    assert not bad, f"(pass, batch, differing bytes of the array or of its SHA-256): {bad}"
