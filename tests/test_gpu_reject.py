"""Truncated sampling on the device (df_flow_sample_region, flows.sample_with_rejection —
src/Flows.jl:196-229).

Every expectation is built by tests/reject_ref.py (pinned on literals in
tests/test_reject_host.py) from candidates that HIPChain.run_sample returns, and every
comparison is bitwise.  `cfg2` runs the FAST SPLIT kernel at every batch size, whose output
for a sample does not depend on the batch (tests/test_gpu_batch_edges.py), so its candidates
come from one run_sample call.  `readme` takes the small-batch kernel for small rounds and the
FAST kernel for large ones; its candidates are drawn with one run_sample call per round, of
the size and at the stream offset the library uses, and nothing is asserted across the two
families.  Output buffers are 64 rows longer than n_want and pre-filled with one NaN bit
pattern that must survive in the pad and in every slot that was not filled.
"""
import numpy as np
import pytest

import densityflows_amd as dfa
from densityflows_amd import _lib
from densityflows_amd.data import MetaData
from helpers import spec_to_element
import reject_ref as R
from test_gpu_train import SPECS

pytestmark = pytest.mark.gpu

NAN32 = 0x7FC0DEAD
PAD = 64
SEED = 5
THETA = {"readme": (0.3,), "cfg2": ()}
INF = np.float32(np.inf)


class _Case:
    """A fresh model and df_chain of SPECS[name] (weights from default_rng(0)) and its Flow."""

    def __init__(self, name, cuda):
        import torch

        make, self.d, self.n = SPECS[name]
        self.name, self.dev = name, cuda
        self.model = spec_to_element(make(np.random.default_rng(0)))
        self.flow = dfa.Flow(self.model, metadata=MetaData("", self.d, self.n, np.zeros(self.n, np.float32),
                                                           np.ones(self.n, np.float32)))
        self.h = self.flow.hip()
        self.theta = THETA[name]
        self.thvec = torch.tensor(self.theta, dtype=torch.float32, device=cuda) if self.n else None

    def candidates(self, N, seed=SEED, offset=0):
        """run_sample → (d, N) numpy: candidates 0..N-1 of the (seed, offset) stream in one batch."""
        import torch

        buf = torch.empty(N * self.d, dtype=torch.float32, device=self.dev)
        self.h.run_sample(buf, self.thvec, self.n > 0, N, seed, offset)
        return buf.cpu().numpy().reshape(N, self.d).T.copy()

    def region_call(self, n_want, arrays, max_tries, round, seed=SEED, offset=0):
        """df_flow_sample_region into a guarded buffer → (rows (d, n_want) as int32 bits, tried,
        accepted, the ArgumentError or None).  The pad is checked."""
        import torch

        out = torch.full(((n_want + PAD) * self.d,), NAN32, dtype=torch.int32, device=self.dev)
        err = None
        try:
            tried, acc = self.h.run_sample_region(out.view(torch.float32), self.thvec, n_want, *arrays, max_tries,
                                                  round, seed, offset)
        except _lib.ArgumentError as e:
            err, tried, acc = e, e.tried, e.accepted
        torch.cuda.synchronize()
        raw = out.cpu().numpy().reshape(n_want + PAD, self.d)
        assert np.all(raw[n_want:] == NAN32), f"{self.name}: written past the {n_want} rows of x_out"
        return raw[:n_want].T.copy(), tried, acc, err


_CASES = {}


def _case(name, cuda):
    """One shared chain per name (the cached candidates below are never modified)."""
    if name not in _CASES:
        _CASES[name] = _Case(name, cuda)
    return _CASES[name]


_ROUNDS = {}


def _stream(C, round, need, max_tries, arrays, seed=SEED, offset=0):
    """The candidates the library examines, as it cuts them: with `round` None one batch
    (cfg2: batch-independent kernels), else one run_sample per round of that size at Philox
    counter offset + d·k0/4.  Extended until `need` of them pass `arrays` or max_tries is
    covered; cached per (chain, round, seed, offset)."""
    key = (C.name, round, seed, offset)
    x = _ROUNDS.get(key, np.zeros((C.d, 0), np.float32))
    while True:
        if x.shape[1] >= max_tries or int(R.predicate(x, *arrays)[:max_tries].sum()) >= need:
            return x
        if round is None:
            x = C.candidates(max(8192, 2 * x.shape[1]), seed, offset)
        else:
            k0 = x.shape[1]
            assert k0 % 4 == 0
            x = np.concatenate([x, C.candidates(round, seed, offset + C.d * (k0 // 4))], axis=1)
        _ROUNDS[key] = x


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


_BOX = {}


def _box(C):
    """(lo, hi, A, b) of a box with acceptance near one half: quantiles of a seeded sample of
    4096 points, two-sided in the first four dimensions and open below in the last.  The
    reference's own acceptance over 4096 candidates of the tests' stream must lie in
    [0.2, 0.8], so a mis-built box fails here and nothing passes vacuously."""
    if C.name not in _BOX:
        x = dfa.sample(C.flow, 4096, C.theta if C.n else None, seed=11).cpu().numpy()
        lo = np.quantile(x, 0.07, axis=1).astype(np.float32)
        hi = np.quantile(x, 0.93, axis=1).astype(np.float32)
        lo[-1] = -INF
        arrays = dfa.Region(dfa.Box(lo, hi)).arrays(C.d)
        rate = R.predicate(_stream(C, None, 1 << 30, 4096, arrays)[:, :4096], *arrays).mean()
        print(f"BOX {C.name}: acceptance {rate:.3f}")
        assert 0.2 <= rate <= 0.8, (C.name, rate)
        _BOX[C.name] = arrays
    return _BOX[C.name]


def _check(C, arrays, n_want, round, max_tries=None, ref_round="same", seed=SEED, offset=0):
    """One call against reject_ref → (rows bits, tried, accepted)."""
    max_tries = 100 * n_want if max_tries is None else max_tries
    if ref_round == "same":
        ref_round = None if C.name == "cfg2" else (round + 3) // 4 * 4
    x = _stream(C, ref_round, n_want, max_tries, arrays, seed, offset)
    want, w_tried, w_acc = R.first_accepted(x, R.predicate(x, *arrays), n_want, max_tries)
    got, tried, acc, err = C.region_call(n_want, arrays, max_tries, round, seed, offset)
    assert (tried, acc) == (w_tried, w_acc), (C.name, n_want, round, (tried, acc), (w_tried, w_acc))
    assert (err is None) == (acc == n_want)
    np.testing.assert_array_equal(got[:, :acc], _bits(want))
    assert np.all(got[:, acc:] == NAN32)
    return got, tried, acc


PARITY = [(n, r) for n in (1, 63, 64, 65, 1000) for r in (4, 64, 260, 70000) if r != 4 or n <= 65]
PARITY.append((1000, 300000))


@pytest.mark.parametrize("n_want,round", PARITY)
@pytest.mark.parametrize("name", ["cfg2", "readme"])
def test_parity(cuda, name, n_want, round):
    """Samples, tried and accepted against reject_ref.  260 leaves a workgroup of one partial
    wave.  The scan walks 1024 ballots per trip, four per thread: 70000 candidates are 1094
    ballots, two trips with a carry and a thread whose four are cut by the round's end;
    300000 are 4688, five trips.  At n_want = 1000 and round = 260 the last slot fills inside
    a round and inside a wave that holds further accepted candidates, which the
    slot < n_want cut must leave out."""
    C = _case(name, cuda)
    got, tried, acc = _check(C, _box(C), n_want, round)
    assert acc == n_want and n_want <= tried <= 5 * n_want + 40
    if (n_want, round) == (1000, 260):
        x = _stream(C, None if name == "cfg2" else round, n_want, 100 * n_want, _box(C))
        k = (tried - 1) % round                       # the filling candidate inside its round
        wave_end = tried - 1 - k + min((k // 64 + 1) * 64, round)
        assert R.predicate(x[:, tried:wave_end], *_box(C)).any(), "no accepted candidate after the last slot's"


def test_round_invariance_cfg2(cuda):
    C = _case("cfg2", cuda)
    outs = [C.region_call(1000, _box(C), 100000, r) for r in (64, 260, 70000, 0)]
    for got, tried, acc, err in outs[1:]:
        assert err is None and (tried, acc) == outs[0][1:3]
        np.testing.assert_array_equal(got, outs[0][0])
    _check(C, _box(C), 1000, 0)


@pytest.mark.parametrize("name", ["cfg2", "readme"])
def test_offset_moves_the_stream(cuda, name):
    C = _case(name, cuda)
    a, _, _ = _check(C, _box(C), 65, 64, offset=0)
    b, _, _ = _check(C, _box(C), 65, 64, offset=1000)
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("name", ["cfg2", "readme"])
def test_accept_all_is_sample(cuda, name):
    """An infinite box and no half-spaces: bitwise sample(flow, n, θ, seed), in one round of n."""
    C = _case(name, cuda)
    n = 1000
    want = dfa.sample(C.flow, n, C.theta if C.n else None, seed=SEED).cpu().numpy()
    got, tried, acc = dfa.sample_with_rejection(dfa.Region(), C.flow, n, C.theta, seed=SEED, round=n,
                                                return_counts=True)
    assert (tried, acc) == (n, n) and tuple(got.shape) == (C.d, n)
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    rows, tried, acc, err = C.region_call(n, dfa.Region().arrays(C.d), 100 * n, n)
    assert err is None and (tried, acc) == (n, n)
    np.testing.assert_array_equal(rows, _bits(want))


def _halfspaces(C, h, q):
    """h constraints with coefficients of mixed sign and magnitude; b[h] the q-quantile of
    a[h]·x over 4096 candidates, so each constraint alone accepts about q."""
    rng = np.random.default_rng(17)
    A = (rng.standard_normal((h, C.d)) * 10.0 ** rng.integers(-3, 4, size=(h, 1))).astype(np.float32)
    x = _stream(C, None, 1 << 30, 4096, dfa.Region().arrays(C.d))[:, :4096].astype(np.float64)
    b = np.quantile(A.astype(np.float64) @ x, q, axis=1).astype(np.float32)
    assert (A > 0).any() and (A < 0).any()
    assert h == 1 or np.abs(A).max() / np.abs(A).min() > 1e3   # rows of different magnitude
    return dfa.HalfSpaces(A, b)


@pytest.mark.parametrize("h,q,boxed", [(1, 0.5, False), (8, 0.92, False), (3, 0.85, True)])
def test_halfspaces_cfg2(cuda, h, q, boxed):
    C = _case("cfg2", cuda)
    box = None
    if boxed:
        lo, hi, _, _ = _box(C)
        box = dfa.Box(np.where(np.arange(C.d) < 2, lo, -INF), np.where(np.arange(C.d) < 2, hi, INF))
    arrays = dfa.Region(box, _halfspaces(C, h, q)).arrays(C.d)
    x = _stream(C, None, 1 << 30, 4096, arrays)[:, :4096]
    rate = R.predicate(x, *arrays).mean()
    print(f"HALFSPACES h={h} boxed={boxed}: acceptance {rate:.3f}")
    assert 0.2 <= rate <= 0.8, rate
    for n_want, round in ((65, 64), (1000, 260), (1000, 0)):
        _check(C, arrays, n_want, round)


def test_exhaustion_empty_box(cuda):
    """max_tries = 1001 is clipped inside a round: tried is 1001, not 1004."""
    C = _case("cfg2", cuda)
    with pytest.raises(dfa.ArgumentError, match="Impossible to reach convergence of rejection sampling") as ei:
        dfa.sample_with_rejection(dfa.Box(1, 0), C.flow, 1001, C.theta, m=1, seed=SEED)
    assert (ei.value.tried, ei.value.accepted) == (1001, 0)
    for round in (0, 4, 260):
        got, tried, acc, err = C.region_call(1001, dfa.Box(1, 0).arrays(C.d) + dfa.Region().arrays(C.d)[2:], 1001,
                                             round)
        assert err is not None and (tried, acc) == (1001, 0) and np.all(got == NAN32)


@pytest.mark.parametrize("name", ["cfg2", "readme"])
def test_exhaustion_keeps_the_filled_rows(cuda, name):
    """max_tries stops right before the 11th acceptance: 10 of 20 slots are filled, equal to
    the reference's, and the other 10 rows still hold the pre-filled pattern."""
    C = _case(name, cuda)
    arrays = _box(C)
    round = 64
    x = _stream(C, None if name == "cfg2" else round, 11, 4096, arrays)
    max_tries = int(np.flatnonzero(R.predicate(x, *arrays))[10])
    got, tried, acc = _check(C, arrays, 20, round, max_tries=max_tries)
    assert (tried, acc) == (max_tries, 10)
    # and with one candidate more the 11th is taken
    got, tried, acc = _check(C, arrays, 20, round, max_tries=max_tries + 1)
    assert (tried, acc) == (max_tries + 1, 11)


@pytest.mark.parametrize("name,round", [("cfg2", 0), ("readme", 64), ("readme", 0)])
def test_region_against_closure(cuda, name, round):
    """The callable path with a closure stating the same box: the same arrays and counts."""
    C = _case(name, cuda)
    lo, hi, _, _ = _box(C)
    seen = []

    def condition(x, theta):
        seen.append((x.dtype, x.shape, theta))
        return bool(np.all(lo <= x) and np.all(x <= hi))

    a = dfa.sample_with_rejection(dfa.Box(lo, hi), C.flow, 65, C.theta, seed=SEED, round=round, return_counts=True)
    b = dfa.sample_with_rejection(condition, C.flow, 65, C.theta, seed=SEED, round=round, return_counts=True)
    assert a[1:] == b[1:] and a[2] == 65
    np.testing.assert_array_equal(_bits(a[0].cpu().numpy()), _bits(b[0].cpu().numpy()))
    assert len(seen) == a[1] and seen[0] == (np.float32, (C.d,), C.theta)
    # the closure path runs out as the region path does
    with pytest.raises(dfa.ArgumentError, match="Impossible to reach convergence") as ei:
        dfa.sample_with_rejection(lambda x, th: False, C.flow, 3, C.theta, m=7, seed=SEED, round=round)
    assert (ei.value.tried, ei.value.accepted) == (21, 0)


def test_dims_tuple_shape(cuda):
    C = _case("readme", cuda)
    box = dfa.Box(*_box(C)[:2])
    r = dfa.sample_with_rejection(box, C.flow, (2, 5, 7), C.theta, seed=SEED, round=64)
    flat = dfa.sample_with_rejection(box, C.flow, 70, C.theta, seed=SEED, round=64)
    assert tuple(r.shape) == (5, 2, 5, 7) and tuple(flat.shape) == (5, 70)
    np.testing.assert_array_equal(_bits(r.cpu().numpy().reshape(5, 70, order="F")), _bits(flat.cpu().numpy()))
    assert tuple(dfa.sample_with_rejection(box, C.flow, (0,), C.theta, seed=SEED).shape) == (5, 0)
    assert tuple(dfa.sample_with_rejection(box, C.flow, (), C.theta, seed=SEED).shape) == (5,)


@pytest.mark.parametrize("name", ["cfg2", "readme"])
def test_workspace_growth_and_other_calls_unchanged(cuda, name):
    """Two calls on one chain with different n_want give what fresh chains give (the second
    grows the workspaces); sample and logpdf after them are bitwise what they were before."""
    import torch

    shared = _Case(name, cuda)
    arrays = _box(_case(name, cuda))
    th = shared.theta if shared.n else None
    s0 = dfa.sample(shared.flow, 1000, th, seed=3).cpu().numpy()
    lp0 = dfa.logpdf(shared.flow, s0, th)
    first = shared.region_call(64, arrays, 6400, 0)
    second = shared.region_call(3000, arrays, 300000, 0)
    third = shared.region_call(64, arrays, 6400, 0)
    for got, n_want in ((first, 64), (second, 3000)):
        fresh = _Case(name, cuda).region_call(n_want, arrays, 100 * n_want, 0)
        assert got[3] is None and got[1:3] == fresh[1:3]
        np.testing.assert_array_equal(got[0], fresh[0])
    assert third[1:3] == first[1:3]
    np.testing.assert_array_equal(third[0], first[0])
    s1 = dfa.sample(shared.flow, 1000, th, seed=3).cpu().numpy()
    np.testing.assert_array_equal(_bits(s1), _bits(s0))
    np.testing.assert_array_equal(_bits(dfa.logpdf(shared.flow, s0, th)), _bits(lp0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["cfg2", "readme"])
def test_repeatable(cuda, name):
    C = _case(name, cuda)
    a = C.region_call(1000, _box(C), 100000, 0)
    b = C.region_call(1000, _box(C), 100000, 0)
    assert a[3] is None and a[1:3] == b[1:3]
    np.testing.assert_array_equal(a[0], b[0])


def test_device_side_argument_checks(cuda):
    import torch

    C = _case("readme", cuda)
    lo, hi, A, b = dfa.Region().arrays(4)
    with pytest.raises(dfa.DimensionMismatch, match="the flow's d"):
        C.region_call(4, (lo, hi, A, b), 400, 0)
    out = torch.full((20,), NAN32, dtype=torch.int32, device=cuda)
    with pytest.raises(dfa.DimensionMismatch, match="θ must match"):       # θ missing: df_flow_sample's words
        C.h.run_sample_region(out.view(torch.float32), None, 4, *dfa.Region().arrays(5), 400, 0, SEED)
    assert C.h.run_sample_region(out.view(torch.float32), C.thvec, 0, *dfa.Region().arrays(5), 0, 0, SEED) == (0, 0)
    # max_tries = 0: nothing is examined
    with pytest.raises(dfa.ArgumentError) as ei:
        C.h.run_sample_region(out.view(torch.float32), C.thvec, 4, *dfa.Region().arrays(5), 0, 0, SEED)
    assert (ei.value.tried, ei.value.accepted) == (0, 0)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == NAN32)
