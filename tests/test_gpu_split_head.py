"""The head of a net body of the specialised SPLIT kernel (densityflows.jl_amd/csrc/
df_uniform_impl.h, net_tiles' read-ahead path): the per-layer slot words and the net's
stage offset come from scalar registers loaded once per net, the hidden and output
offsets are derived from the stage offset, and the first-Dense fragments, the features
and step 0 of the hidden Dense are one LDS request.  Only loads, waits and registers
moved, so:

1. every pass on every model of tests/golden/make_head_pin.py gives the pinned bits of
   tests/golden/head_pin_*.npz (the generator states the commit they come from), at
   DF_TILES unset, 2 and — where the plan holds four tiles — 4 (two tile groups per net);
   forward! gives forward's pinned x;
2. the launches ran the specialised SPLIT kernel with the tiles per wave the setting means;
3. repeated launches on the same inputs give the same bits (a read that raced with a
   write of the stage buffer or of the state rows would not)."""
import re

import numpy as np
import pytest

import make_head_pin as P

pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"\[df\] mode (\d+) batch (\d+) kernel (\S+) tiles (\d+) \(max (\d+)\)")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cases():
    return [(name, forced) for name in sorted(P.MODELS) for forced, _ in P.tile_settings(name)]


def _handle(name, forced, monkeypatch):
    monkeypatch.delenv("DF_TILES", raising=False)
    monkeypatch.setenv("DF_DEBUG_LAUNCH", "1")
    if forced:
        monkeypatch.setenv("DF_TILES", forced)
    return P.compile_model(name)


@pytest.mark.parametrize("name,forced", _cases())
def test_pinned_bits(cuda, monkeypatch, capfd, name, forced):
    tiles = dict(P.tile_settings(name))[forced]
    want = np.load(P.path(name))
    hc = _handle(name, forced, monkeypatch)
    assert hc.info.kernel == 4, hc.info.kernel
    capfd.readouterr()
    bad = []
    for B in P.batches(tiles):
        got = P.passes(hc, name, B)
        for k in P.PASSES + ("fwdi_x",):
            w = want[f"{'fwd_x' if k == 'fwdi_x' else k}_{B}"]
            assert got[k].shape == w.shape, (k, B)
            n = int(np.sum(_bits(got[k]) != _bits(w)))
            if n:
                bad.append((k, B, n))
    ran = LAUNCH.findall(capfd.readouterr().err)
    assert len(ran) == 4 * len(P.batches(tiles)), ran
    for _, batch, kernel, t, max_t in ran:
        assert int(t) == tiles, f"{name} DF_TILES={forced}: batch {batch} ran {t} tiles per wave (kernel {kernel})"
        assert int(max_t) == P.MAX_TILES[name], (name, max_t)
    assert not bad, f"(pass, batch, differing words): {bad}"


@pytest.mark.parametrize("name", sorted(P.MODELS))
def test_repeated_launches_same_bits(cuda, monkeypatch, name):
    forced, tiles = P.tile_settings(name)[-1]
    hc = _handle(name, forced, monkeypatch)
    S = P.samples_per_block(tiles)
    for B in (S + 1, 2 * S + 33):
        first = P.passes(hc, name, B)
        for rep in (1, 2):
            again = P.passes(hc, name, B)
            for k in first:
                assert np.array_equal(_bits(again[k]), _bits(first[k])), (k, B, rep)
