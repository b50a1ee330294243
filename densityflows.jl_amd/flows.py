"""Flow / density API — mirror of src/Flows.jl and the @flow_wrapper methods
(src/Macros.jl:104-112): θ is normalised with the Flow's MetaData inside the
fused kernel (df_flow_* entry points).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .chains import FlowChain, _n_of
from .data import DataArrays, MetaData, maximum_theta, minimum_theta
from .hip import as_julia_device, julia_empty

__all__ = ["Flow", "MvNormal", "predict", "sample", "sample_logpdf", "sample_with_rejection", "Box", "HalfSpaces",
           "Region", "logpdf", "logpdf_grid", "logpdf_grad", "pdf", "pdf_marginals", "trapezoid_weights",
           "training_loss", "validation_loss", "nll_partial_sum", "ScoreMoments", "score_moments",
           "fisher_information", "entropy", "hpd_levels", "expected_coverage", "PointStats", "posterior_stats",
           "sbc_ranks", "sbc_histogram", "QUANT_MAX_ORDERS", "quantile_orders", "order_statistics",
           "posterior_quantiles", "credible_intervals", "HIST_MAX_BINS", "HIST_MAX_TABLES", "HIST_SPLIT_DRAWS",
           "histogram_edges", "draw_histograms", "posterior_histograms", "PointHistograms", "posterior_draws",
           "ImportanceWeights", "importance_weights", "WeightedPointStats", "weighted_moments_from_sums",
           "weighted_stats", "importance_posterior_stats", "RESAMPLE_METHODS", "RESAMPLE_LDS_DRAWS",
           "resample_indices", "resample", "importance_resample", "WQUANT_MAX_PROBS", "WHIST_MAX_TABLE_BINS",
           "quantile_numerators", "weight_scale", "weighted_quantiles", "weighted_credible_intervals",
           "WeightedPointHistograms", "weighted_histograms", "importance_posterior_quantiles",
           "importance_credible_intervals", "importance_posterior_histograms"]

LOG2PI = float(np.log(2.0 * np.pi))


class MvNormal:
    """Base distribution ``MvNormal(zeros(d), I)`` — src/Flows.jl:114 (the only
    base the fused logpdf supports)."""

    def __init__(self, d: int):
        self.d = d

    def __repr__(self):
        return f"MvNormal(0, I_{self.d})"


class Flow:
    """``Flow([base, ] model, data)`` — src/Flows.jl:37-122."""

    def __init__(self, model: FlowChain, data: Optional[DataArrays] = None, base=None, metadata: MetaData = None,
                 train_loss=None, valid_loss=None):
        if not isinstance(model, FlowChain):
            raise _lib.ArgumentError("Flow needs a FlowChain model")
        if metadata is None:
            if data is None:
                raise _lib.ArgumentError("Flow needs DataArrays (or explicit MetaData)")
            d, n = data.number_dimensions(), data.number_conditions()
            metadata = MetaData("", d, n, np.asarray(minimum_theta(data), np.float32),
                                np.asarray(maximum_theta(data), np.float32))
        self.model = model
        self.metadata = metadata
        self.base = base if base is not None else MvNormal(metadata.d)
        if not isinstance(self.base, MvNormal):
            raise _lib.UnsupportedError("only the standard MvNormal base is fused on device")
        self.train_loss = list(train_loss or [])
        self.valid_loss = list(valid_loss or [])

    @property
    def d(self):
        return self.metadata.d

    @property
    def n(self):
        return self.metadata.n

    def hip(self, device=None):
        h = self.model.hip(device=device, n_hint=self.n)
        if self.n > 0 and h.bounds is None:
            h.set_theta_bounds(self.metadata.theta_min, self.metadata.theta_max)
        return h

    def summarize(self) -> str:
        return ("- model --------------------\n" + self.model.summarize() +
                "\n- base distribution --------\nMvNormal")

    # @flow_wrapper backward forward forward!  (src/DensityFlows.jl:72)
    def forward(self, z, theta=None):
        return self.hip().apply("forward", z, self._theta(theta, z), flow=True)

    def backward(self, x, theta=None):
        return self.hip().apply("backward", x, self._theta(theta, x), flow=True)

    def forward_(self, z, theta=None):
        return self.hip().apply_inplace(z, self._theta(theta, z), flow=True)

    def _theta(self, theta, y, device: bool = False):
        """θ as the array-level call takes it.  An NTuple θ is broadcast to (n, dims...):
        ``device=True`` (logpdf, pdf, nll_partial_sum) leaves it on the device, filled by
        ``df_theta_broadcast``; otherwise it comes back as ``y`` is (numpy for numpy)."""
        if self.n == 0:
            return None
        if theta is None:
            raise _lib.DimensionMismatch("dimensions θ must match (n, dims...) with n number of trained parameters")
        if isinstance(theta, tuple):  # NTuple θ: one condition for every point
            if device:
                return _broadcast_theta_device(self.hip(), theta, tuple(y.shape[1:]), y)
            return _broadcast_theta(theta, tuple(y.shape[1:]), y)
        return theta


def _broadcast_theta(theta: tuple, dims, like):
    """``collect(θ) .* ones(T, (1, dims...))`` — src/Flows.jl:182."""
    import torch

    dev = like.device if isinstance(like, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    buf, view = julia_empty(len(theta), tuple(dims), dev)
    t = torch.tensor([float(np.float32(v)) for v in theta], dtype=torch.float32, device=dev)
    buf.view(-1, len(theta)).copy_(t.expand(buf.numel() // len(theta), len(theta)))
    if not isinstance(like, torch.Tensor):
        return view.cpu().numpy()
    return view


def _broadcast_theta_device(h, theta: tuple, dims, like):
    """``_broadcast_theta`` without the host: the (n, dims...) array stays a device tensor."""
    import torch

    dev = like.device if isinstance(like, torch.Tensor) and like.device.type == "cuda" else h.device
    buf, view = julia_empty(len(theta), tuple(dims), dev)
    t = torch.tensor([float(np.float32(v)) for v in theta], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        h.run_theta_broadcast(buf, t, buf.numel() // max(len(theta), 1))
    return view


def predict(flow: Flow, z, theta=None):
    """``predict(flow, z, θ) = forward(flow, z, θ)[1]`` — src/Flows.jl:126."""
    return flow.forward(z, theta)[0]


def sample(flow: Flow, dims: Union[int, Tuple[int, ...]], theta=None, rng=None, seed: Optional[int] = None,
           offset: int = 0):
    """``sample([rng, ] flow, dims [, θ])`` — src/Flows.jl:157-192, one library call
    (``df_flow_sample``): r ~ MvNormal(0, I) drawn on the device from a Philox4x32-10
    stream keyed by ``seed`` (default: 64 bits drawn from ``rng``, a
    ``numpy.random.Generator``, as Julia draws from its ``rng``; Julia's Xoshiro
    stream itself is not reproduced), shape (d, dims...) in Julia memory order,
    then the fused ``forward!`` with θ normalised in the kernel.  θ: an array
    (n, dims...) or an NTuple broadcast to every point (Flows.jl:178-188)."""
    import torch

    if isinstance(dims, int):
        dims = (dims,)
    dims = tuple(int(v) for v in dims)
    if seed is None:
        rng = rng if rng is not None else np.random.default_rng()
        seed = int(rng.integers(0, 2**63 - 1, dtype=np.int64)) * 2 + int(rng.integers(0, 2))
    h = flow.hip()
    dev = h.device
    buf, r = julia_empty(flow.d, dims, dev)
    batch = int(np.prod(dims)) if dims else 1
    thb, bcast = None, False
    if flow.n > 0:
        if theta is None:
            raise AssertionError("dimensions θ must match (n, dims...) with n number of trained parameters")
        if isinstance(theta, tuple):
            if len(theta) != flow.n:
                raise AssertionError("dimensions θ must match (n, dims...) with n number of trained parameters")
            thb = torch.tensor([float(np.float32(v)) for v in theta], dtype=torch.float32, device=dev)
            bcast = True
        else:
            if tuple(theta.shape) != (flow.n,) + dims:
                raise AssertionError("dimensions θ must match (n, dims...) with n number of trained parameters")
            thb, _, _ = as_julia_device(theta, flow.n, dev, "θ")
    h.run_sample(buf, thb, bcast, batch, seed, offset)
    return r


def sample_logpdf(flow: Flow, dims: Union[int, Tuple[int, ...]], theta=None, rng=None, seed: Optional[int] = None,
                  offset: int = 0):
    """``(x, lp)``: a draw like :func:`sample`'s together with ``lp = log q(x | θ)`` of every
    drawn point, shapes (d, dims...) and (dims...), from ONE forward pass per sample
    (``df_flow_sample_logpdf``): the base log-density of the draw minus the forward ldj, where
    ``sample`` then ``logpdf`` runs a forward and a full inverse pass.  Arguments as for
    :func:`sample`.  ``x`` is ``forward`` of the ``(seed, offset)`` draw; ``sample`` runs
    ``forward!`` on the same draw, and the two are not promised to agree bit for bit."""
    import torch

    from .hip import HIPChain

    if isinstance(dims, int):
        dims = (dims,)
    dims = tuple(int(v) for v in dims)
    bad = AssertionError("dimensions θ must match (n, dims...) with n number of trained parameters")
    if flow.n > 0:
        if theta is None or (isinstance(theta, tuple) and len(theta) != flow.n):
            raise bad
        if not isinstance(theta, tuple) and tuple(theta.shape) != (flow.n,) + dims:
            raise bad
    seed = _draw_seed(rng, seed)
    h = flow.hip()
    dev = h.device
    buf, r = julia_empty(flow.d, dims, dev)
    batch = int(np.prod(dims)) if dims else 1
    lpb = torch.empty(batch, dtype=torch.float32, device=dev)
    thb, bcast = None, False
    if flow.n > 0:
        if isinstance(theta, tuple):
            thb, bcast = _theta_vector(theta, dev), True
        else:
            thb, _, _ = as_julia_device(theta, flow.n, dev, "θ")
    h.run_sample_logpdf(buf, lpb, thb, bcast, batch, seed, offset)
    return r, HIPChain._ldj_view(lpb, dims)


def _draw_seed(rng, seed: Optional[int]) -> int:
    """The 64-bit Philox key: ``seed``, or 64 bits drawn from ``rng`` as :func:`sample` draws them."""
    if seed is not None:
        return int(seed)
    rng = rng if rng is not None else np.random.default_rng()
    return int(rng.integers(0, 2**63 - 1, dtype=np.int64)) * 2 + int(rng.integers(0, 2))


def _theta_vector(theta: tuple, dev):
    import torch

    return torch.tensor([float(np.float32(v)) for v in theta], dtype=torch.float32, device=dev)


# ---------------------------------------------------------------------------
# truncated sampling — src/Flows.jl:196-229
# ---------------------------------------------------------------------------

def _f32_no_nan(a, what):
    a = np.asarray(a, dtype=np.float32)
    if np.isnan(a).any():
        raise _lib.ArgumentError(f"NaN in {what}")
    return a


class Box:
    """``lo[k] <= x[k] <= hi[k]`` in every dimension; ±inf allowed; a scalar bound holds for
    every dimension.  ``lo > hi`` is legal: the box is empty."""

    def __init__(self, lo=-np.inf, hi=np.inf):
        self.lo, self.hi = _f32_no_nan(lo, "the box's lo"), _f32_no_nan(hi, "the box's hi")
        for v, name in ((self.lo, "lo"), (self.hi, "hi")):
            if v.ndim > 1:
                raise _lib.DimensionMismatch(f"the box's {name} must be a scalar or a vector of d values")
        if self.lo.ndim == 1 and self.hi.ndim == 1 and self.lo.shape != self.hi.shape:
            raise _lib.DimensionMismatch("the box's lo and hi differ in length")

    def arrays(self, d: int):
        out = []
        for v, name in ((self.lo, "lo"), (self.hi, "hi")):
            if v.ndim == 1 and v.shape[0] != d:
                raise _lib.DimensionMismatch(f"the box's {name} has {v.shape[0]} values, the flow has d = {d}")
            out.append(np.ascontiguousarray(np.broadcast_to(v, (d,)), dtype=np.float32))
        return tuple(out)


class HalfSpaces:
    """``Σ_k A[h, k]·x[k] <= b[h]`` for each of up to 8 rows of ``A`` (h, d); one constraint
    may be given as a vector and a scalar.  The sum is taken left to right in Float32."""

    def __init__(self, A, b):
        A, b = _f32_no_nan(A, "the half-spaces' A"), _f32_no_nan(b, "the half-spaces' b")
        if A.ndim == 1 and b.ndim == 0:
            A, b = A[None, :], b[None]
        if A.ndim != 2 or b.ndim != 1 or A.shape[0] != b.shape[0]:
            raise _lib.DimensionMismatch("half-spaces need A of size (h, d) and b of h values")
        if A.shape[0] > _lib.DF_REGION_MAX_HALFSPACES:
            raise _lib.UnsupportedError(f"a region holds at most {_lib.DF_REGION_MAX_HALFSPACES} half-spaces")
        if A.shape[0] > 0 and A.shape[1] < 1:
            raise _lib.DimensionMismatch("half-spaces need A of size (h, d) with d >= 1")
        self.A, self.b = np.ascontiguousarray(A), np.ascontiguousarray(b)

    def arrays(self, d: int):
        if self.A.shape[0] > 0 and self.A.shape[1] != d:
            raise _lib.DimensionMismatch(f"the half-spaces' A has {self.A.shape[1]} columns, the flow has d = {d}")
        return self.A.reshape(-1, d), self.b


class Region:
    """A :class:`Box` and / or :class:`HalfSpaces`: the ``condition`` of
    :func:`sample_with_rejection` that is evaluated on the device."""

    def __init__(self, box: Optional[Box] = None, halfspaces: Optional[HalfSpaces] = None):
        if box is not None and not isinstance(box, Box):
            raise _lib.ArgumentError("Region: box must be a Box")
        if halfspaces is not None and not isinstance(halfspaces, HalfSpaces):
            raise _lib.ArgumentError("Region: halfspaces must be a HalfSpaces")
        self.box, self.halfspaces = box, halfspaces

    def arrays(self, d: int):
        """(lo (d), hi (d), A (h, d), b (h)) in Float32, as the library takes them."""
        lo, hi = (self.box if self.box is not None else Box()).arrays(d)
        if self.halfspaces is not None:
            A, b = self.halfspaces.arrays(d)
        else:
            A, b = np.zeros((0, d), np.float32), np.zeros(0, np.float32)
        return lo, hi, A, b


# df_reject.hip's adaptive schedule (round = 0), restated: the closure path cuts the
# candidate stream where the library does
_REJ_MIN_ROUND, _REJ_MAX_ROUND = 1 << 10, 1 << 22


def _round_up4(v: int) -> int:
    return (v + 3) // 4 * 4


def _first_round(n_want: int) -> int:
    return _round_up4(min(max(2 * min(n_want, _REJ_MAX_ROUND), _REJ_MIN_ROUND), _REJ_MAX_ROUND))


def _next_round(remaining: int, examined: int, accepted: int, prev: int) -> int:
    want = 2 * prev if accepted == 0 else -(-(remaining * examined * 5) // (accepted * 4)) + 64
    return _round_up4(min(max(want, _REJ_MIN_ROUND), _REJ_MAX_ROUND))


def _reject_closure(h, condition, theta, thb, buf, n_want, max_tries, round, seed, offset):
    """The host form: the library's candidate stream through ``run_sample`` round by round,
    ``condition(x, θ)`` per candidate in order, the first ``n_want`` kept → (tried, accepted)."""
    import torch

    d = h.d
    R = _round_up4(round) if round > 0 else _first_round(n_want)
    k0 = accepted = 0
    out = buf.view(-1, d)
    while k0 < max_tries:
        cand = torch.empty(R * d, dtype=torch.float32, device=h.device)
        h.run_sample(cand, thb, thb is not None, R, seed, offset + d * (k0 // 4))
        rows = cand.cpu().numpy().reshape(R, d)
        count = min(R, max_tries - k0)
        keep = []
        for i in range(count):
            if condition(rows[i], theta):
                keep.append(i)
                if accepted + len(keep) == n_want:
                    break
        if keep:
            out[accepted:accepted + len(keep)].copy_(torch.from_numpy(rows[keep]).to(h.device))
        accepted += len(keep)
        if accepted == n_want:
            return k0 + keep[-1] + 1, accepted
        k0 += count
        if round == 0:
            R = _next_round(n_want - accepted, k0, accepted, R)
    return k0, accepted


def sample_with_rejection(condition, flow: Flow, dims: Union[int, Tuple[int, ...]], theta: tuple = (), m: int = 100,
                          rng=None, seed: Optional[int] = None, offset: int = 0, round: int = 0,
                          return_counts: bool = False):
    """``sample_with_rejection([rng, ] condition, flow, dims, θ [, m])`` — src/Flows.jl:196-229:
    the first prod(dims) samples of the flow at the NTuple θ that satisfy ``condition``,
    shape (d, dims...) in Julia memory order.  Candidate k is column k of
    ``sample(flow, N, θ, seed=seed, offset=offset)``; at most ``m``·prod(dims) candidates are
    examined, and if they do not fill the result an ArgumentError is raised, as the
    reference throws (its ``.tried`` / ``.accepted`` hold the counts).

    ``condition`` is a :class:`Region` (or a :class:`Box` / :class:`HalfSpaces`): one library
    call (``df_flow_sample_region``), predicate and order-preserving compaction on the
    device, one small read-back per round of candidates.  Or the reference's closure
    ``condition(x, θ) -> Bool`` with ``x`` a length-d Float32 vector: a host loop over the
    same candidate stream, for predicates a region cannot state; for a closure that states
    a region's predicate both forms return the same arrays.  ``round``: candidates per round
    (0: chosen from ``dims`` and the acceptance rate so far); the result does not depend on
    it.  ``return_counts``: (x, tried, accepted), tried = 1 + the index of the candidate that
    filled the last slot — accepted / tried estimates the region's probability."""
    import torch

    if isinstance(dims, (int, np.integer)):
        dims = (dims,)
    dims = tuple(int(v) for v in dims)
    if any(v < 0 for v in dims):
        raise _lib.DimensionMismatch("dims must be non-negative")
    if not isinstance(theta, tuple):
        raise _lib.ArgumentError("sample_with_rejection takes θ as an NTuple of n values (one condition for "
                                 "every sample); the reference has no method for an array θ")
    if len(theta) != flow.n:
        raise _lib.DimensionMismatch("dimensions θ must match (n, dims...) with n number of trained parameters")
    if isinstance(condition, (Box, HalfSpaces)):
        condition = Region(condition, None) if isinstance(condition, Box) else Region(None, condition)
    if isinstance(condition, Region):
        region = condition.arrays(flow.d)
    elif callable(condition):
        region = None
    else:
        raise _lib.ArgumentError("condition must be a Region, a Box, HalfSpaces or a callable condition(x, θ)")
    m, round, offset = int(m), int(round), int(offset)
    if m < 0 or round < 0:
        raise _lib.DimensionMismatch("m and round must be non-negative")
    if seed is None:
        rng = rng if rng is not None else np.random.default_rng()
        seed = int(rng.integers(0, 2**63 - 1, dtype=np.int64)) * 2 + int(rng.integers(0, 2))
    n_want = int(np.prod(dims)) if dims else 1
    max_tries = m * n_want
    h = flow.hip()
    buf, r = julia_empty(flow.d, dims, h.device)
    thb = None
    if flow.n > 0:
        thb = torch.tensor([float(np.float32(v)) for v in theta], dtype=torch.float32, device=h.device)
    tried = accepted = 0
    if n_want > 0:
        with torch.cuda.device(h.device):
            if region is not None:
                tried, accepted = h.run_sample_region(buf, thb, n_want, *region, max_tries, round, seed, offset)
            else:
                tried, accepted = _reject_closure(h, condition, theta, thb, buf, n_want, max_tries, round, seed,
                                                  offset)
                if accepted < n_want:
                    e = _lib.ArgumentError("sample_with_rejection: Impossible to reach convergence of rejection "
                                           f"sampling: {accepted} of {n_want} accepted after {tried} candidates")
                    e.tried, e.accepted = tried, accepted
                    raise e
    return (r, tried, accepted) if return_counts else r


def logpdf(flow: Flow, x, theta=None):
    """``logpdf(flow, x, θ)`` — src/Flows.jl:272-284: backward + base logpdf + ldj (fused)."""
    if isinstance(x, tuple):
        return _logpdf_axes(flow, x, theta)
    th = flow._theta(theta, x, device=True)
    return flow.hip().logpdf(x, th)


def _axis_values(a, what):
    """One grid axis as (values, is_tensor): a float32 vector, numpy or torch."""
    import torch

    if isinstance(a, torch.Tensor):
        if a.dim() != 1:
            raise _lib.DimensionMismatch(f"{what} must be a vector, got size {tuple(a.shape)}")
        return a.detach().to(torch.float32), True
    a = np.asarray(a, dtype=np.float32)
    if a.ndim != 1:
        raise _lib.DimensionMismatch(f"{what} must be a vector, got size {a.shape}")
    return a, False


def _grid_axes(flow: Flow, x_axes, theta_axes):
    """The d + n axes of a grid → (handle, axis vectors, lens, any device tensor?, the axes
    concatenated on the device)."""
    import torch

    h = flow.hip()
    d, n = flow.d, flow.n
    x_axes = tuple(x_axes)
    theta_axes = tuple(theta_axes) if theta_axes is not None else ()
    if len(x_axes) != d:
        raise _lib.DimensionMismatch(f"a grid in x needs d = {d} vectors, got {len(x_axes)}")
    if len(theta_axes) != n:
        raise _lib.DimensionMismatch(f"a grid needs n = {n} entries of θ (values or vectors), got {len(theta_axes)}")
    parts, any_tensor = [], False
    for k, a in enumerate(x_axes):
        v, is_t = _axis_values(a, f"x axis {k + 1}")
        parts.append(v)
        any_tensor = any_tensor or is_t
    for k, a in enumerate(theta_axes):
        if not isinstance(a, torch.Tensor) and np.ndim(a) == 0:
            a = np.asarray([a], dtype=np.float32)       # one value: an axis of length 1
        elif isinstance(a, torch.Tensor) and a.dim() == 0:
            a = a.reshape(1)
        v, is_t = _axis_values(a, f"θ axis {k + 1}")
        parts.append(v)
        any_tensor = any_tensor or is_t
    lens = tuple(int(v.shape[0]) for v in parts)
    if any_tensor:
        axes_buf = torch.cat([v.to(h.device) if isinstance(v, torch.Tensor) else torch.tensor(v, device=h.device)
                              for v in parts]).contiguous()
    else:
        axes_buf = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, np.float32)).to(h.device)
    return h, parts, lens, any_tensor, axes_buf


def _grid_window(lens, first, count):
    """(first, count) of a window of the grid, checked; count None: to the end."""
    P = 1
    for L in lens:
        P *= L
    first = int(first)
    count = P - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > P:
        raise _lib.DimensionMismatch(f"window [{first}, {first + count}) outside the grid of {P} points")
    return first, count


def _grid_eval(flow: Flow, x_axes, theta_axes, first, count, chunk):
    """Shared by logpdf_grid and the tuple-x logpdf → (flat device values, lens, numpy out?,
    whole grid?)."""
    import torch

    h, _, lens, any_tensor, axes_buf = _grid_axes(flow, x_axes, theta_axes)
    whole = first == 0 and count is None
    first, count = _grid_window(lens, first, count)
    lpb = torch.empty(count, dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        h.run_logpdf_grid(axes_buf, lens, first, count, lpb, chunk)
    return lpb, lens, not any_tensor, whole


def logpdf_grid(flow: Flow, x_axes, theta_axes=None, first: int = 0, count: Optional[int] = None, chunk: int = 0):
    """logpdf on the outer product of axis vectors, generated on the device (one library
    call, ``df_flow_logpdf_grid``): ``x_axes`` are d vectors, ``theta_axes`` n entries,
    each one raw θ value or a vector of them — a likelihood surface over θ is a grid with
    x axes of length 1.  Without a window the result has shape (L₁, …, L_d, M₁, …, M_n)
    (M = 1 for a single value), the first axis varying fastest in memory as in the
    reference's ``reshape(…, lens...)`` (src/Flows.jl:303-304).  With ``first`` / ``count``
    it is the flat values of points [first, first + count) of that order: the grid may be
    far larger than memory, only the window is evaluated.  ``chunk``: points per launch
    (0: the library's default).  numpy in, numpy out; any device tensor among the axes
    gives a device tensor."""
    from .hip import HIPChain, _to_numpy

    lpb, lens, was_np, whole = _grid_eval(flow, x_axes, theta_axes, first, count, chunk)
    v = HIPChain._ldj_view(lpb, lens) if whole else lpb
    return _to_numpy(v) if was_np else v


MAX_MARGINALS = 128     # requests of one df_flow_pdf_marginals call


def trapezoid_weights(axis) -> np.ndarray:
    """Trapezoid-rule weights of one axis in float64, from its float32 values: half the end
    interval at the ends, half the distance between the neighbours inside, so that
    ``weights @ f`` is ``numpy.trapz(f, axis)``.  An axis of one value has weight 1 (a slice)."""
    a = np.asarray(axis, dtype=np.float32).astype(np.float64)
    if a.ndim != 1:
        raise _lib.DimensionMismatch(f"an axis must be a vector, got size {a.shape}")
    if a.size <= 1:
        return np.ones(a.size, np.float64)
    w = np.empty(a.size, np.float64)
    w[0] = 0.5 * (a[1] - a[0])
    w[-1] = 0.5 * (a[-1] - a[-2])
    w[1:-1] = 0.5 * (a[2:] - a[:-2])
    return w


def _marginal_requests(keep, lens, d):
    """``keep`` → sorted, distinct tuples of ascending axis numbers."""
    na = len(lens)
    if keep is None:
        xs = [k for k in range(d) if lens[k] > 1]
        keep = [()] + [(a,) for a in xs] + [(a, b) for i, a in enumerate(xs) for b in xs[i + 1:]]
    out = set()
    for K in keep:
        K = (int(K),) if np.ndim(K) == 0 else tuple(int(v) for v in K)
        if len(K) > 2:
            raise _lib.UnsupportedError(f"a marginal keeps at most two axes, got {K}")
        if len(set(K)) != len(K) or any(v < 0 or v >= na for v in K):
            raise _lib.ArgumentError(f"kept axes must be distinct and in [0, {na}), got {K}")
        out.add(tuple(sorted(K)))
    out = sorted(out, key=lambda K: (len(K), K))
    if len(out) > MAX_MARGINALS:
        raise _lib.UnsupportedError(f"at most {MAX_MARGINALS} marginal tables per call, got {len(out)}")
    return out


def pdf_marginals(flow: Flow, x_axes, theta=None, keep=None, weights="trapezoid", first: int = 0,
                  count: Optional[int] = None, chunk: int = 0):
    """Marginal tables of ``pdf`` on the grid of :func:`logpdf_grid`, reduced on the device
    (one library call, ``df_flow_pdf_marginals``): only the tables come back, whatever the
    grid's size.  ``theta``: n entries, values or vectors, as ``theta_axes`` there.

    ``keep``: the tables wanted, each a tuple of 0, 1 or 2 axis numbers (x axes 0 … d-1, then
    the θ axes); every other axis is integrated with its quadrature weights.  ``None`` is the
    corner plot: ``()`` (the total mass), every x axis of more than one value, every pair of
    them.  ``weights``: ``"trapezoid"`` (:func:`trapezoid_weights` of every axis), ``"sum"``
    (all 1) or a tuple of d + n vectors, the caller's own rule.  ``first`` / ``count``: the
    sums over a window of the grid's points only; windows add up.

    Returns ``{(): scalar, (a,): (L_a,), (a, b): (L_a, L_b)}`` in float64, keys sorted; numpy
    in, numpy out (Fortran-ordered), any device tensor among the axes gives device tensors.
    The sums are accumulated with atomic adds: two runs may differ in the last bits."""
    import torch

    h, parts, lens, any_tensor, axes_buf = _grid_axes(flow, x_axes, theta)
    reqs = _marginal_requests(keep, lens, flow.d)
    first, count = _grid_window(lens, first, count)
    if isinstance(weights, str):
        if weights not in ("trapezoid", "sum"):
            raise _lib.ArgumentError(f'weights must be "trapezoid", "sum" or a tuple of vectors, got {weights!r}')
        host = [v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v for v in parts]
        wparts = [trapezoid_weights(v) if weights == "trapezoid" else np.ones(v.shape[0], np.float64) for v in host]
    else:
        wparts = [np.atleast_1d(np.asarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w,
                                           dtype=np.float64)) for w in tuple(weights)]
        if len(wparts) != len(lens) or any(w.ndim != 1 or w.shape[0] != L for w, L in zip(wparts, lens)):
            raise _lib.DimensionMismatch(f"weights must be d + n = {len(lens)} vectors of the axes' lengths {lens}")
    wbuf = torch.from_numpy(np.concatenate(wparts) if wparts else np.zeros(0, np.float64)).to(h.device)
    shapes = [tuple(lens[k] for k in K) for K in reqs]
    sizes = [int(np.prod(s, dtype=np.int64)) for s in shapes]
    out = torch.empty(sum(sizes), dtype=torch.float64, device=h.device)
    with torch.cuda.device(h.device):
        h.run_pdf_marginals(axes_buf, wbuf, lens, first, count, reqs, out, chunk)
    res, at = {}, 0
    flat = out if any_tensor else out.cpu().numpy()
    for K, shape, size in zip(reqs, shapes, sizes):
        t = flat[at:at + size]
        at += size
        if any_tensor:
            res[K] = t.reshape(tuple(reversed(shape))).permute(tuple(reversed(range(len(shape)))))
        else:
            res[K] = np.array(t.reshape(shape, order="F"), order="F")
    return res


def _logpdf_axes(flow: Flow, x: tuple, theta):
    """``logpdf(flow, (x₁, …, x_d) [, (θ₁, …, θ_n)])`` — src/Flows.jl:287-331."""
    from .hip import HIPChain, _to_numpy

    if len(x) != flow.d:
        raise _lib.DimensionMismatch(f"x given as a tuple must hold d = {flow.d} vectors, got {len(x)}")
    if flow.n == 0:
        theta = ()
    elif not isinstance(theta, tuple):
        raise _lib.DimensionMismatch("if x is given as a tuple of vectors, θ must be passed as an NTuple of n values")
    if len(theta) != flow.n or any(np.ndim(v) != 0 for v in theta):
        raise _lib.DimensionMismatch(f"θ must be an NTuple of n = {flow.n} values")
    lpb, lens, was_np, _ = _grid_eval(flow, x, theta, 0, None, 0)
    v = HIPChain._ldj_view(lpb, lens[:flow.d])
    return _to_numpy(v) if was_np else v


def logpdf_grad(flow: Flow, x, theta=None, state=None):
    """``(lp, gx, gθ)``: ``logpdf(flow, x, θ)`` per point and its gradients in ``x`` and in the
    raw ``θ`` — what ``Zygote.gradient((x, θ) -> sum(logpdf(flow, x, θ)), x, θ)`` gives in the
    reference through ``rrule(RNVP_backward)`` (src/affine/RNVP.jl:137-141) and the θ
    normalisation (``grad_normalisation``, src/Data.jl:236-241).  One library call
    (``df_train_logpdf_grad``).  Shapes (dims...), (d, dims...), (n, dims...); numpy in, numpy
    out; an NTuple θ is broadcast and ``gθ`` returned per point.  ``state``: a
    :class:`TrainState` whose trainer (and current parameters) is used; without it a
    temporary trainer is created and destroyed inside the call."""
    import torch

    from .hip import HIPChain, _to_numpy
    from .train import Adam, HIPTrainer

    th = flow._theta(theta, x)
    if state is not None:
        tr, h = state.trainer, state.trainer.chain
    else:
        h = flow.hip()
        # A new trainer starts from the parameters its chain evaluates (df_train_create), and the
        # model may be newer than the chain (weights loaded or edited in Python): hand the chain
        # the model's current ones first.  The library refuses that while another trainer is
        # bound to the chain (it may hold newer parameters than the model): pass it as `state`.
        try:
            h.set_weights(flow.model.layers)
        except _lib.ArgumentError as e:
            raise _lib.ArgumentError(f"logpdf_grad: the flow has a live TrainState, pass it as state= ({e})") from e
        tr = HIPTrainer(h, Adam())
    try:
        xb, thb, dims, batch, was_np = h._inputs(x, th, "x")
        lpb = torch.empty(batch, dtype=torch.float32, device=h.device)
        gxb, gxv = julia_empty(h.d, dims, h.device)
        gtb, gtv = julia_empty(h.n, dims, h.device)
        tr.logpdf_grad(xb, thb, batch, lpb, gxb, gtb if h.n > 0 else None)
        lpv = HIPChain._ldj_view(lpb, dims)
        if state is None:
            torch.cuda.synchronize(h.device)
    finally:
        if state is None:
            tr.close()
    if was_np:
        return _to_numpy(lpv), _to_numpy(gxv), _to_numpy(gtv)
    return lpv, gxv, gtv


# ---------------------------------------------------------------------------
# expectations under the flow, reduced on the device (df_moments.hip)
# ---------------------------------------------------------------------------

MAX_CHUNK = 1 << 24


class ScoreMoments:
    """The raw sums a moment reduction returns, as numpy float64: ``count``, ``lp_sum = Σ lp``,
    ``lp_sqsum = Σ lp²``, ``score_sum = Σ g`` (n,) and ``outer = Σ g gᵀ`` (n, n), with
    ``g = ∂lp/∂θ`` in the raw θ.  The properties are computed on the host in float64."""

    def __init__(self, block, n: int):
        block = np.asarray(block, dtype=np.float64).reshape(-1)
        if block.shape[0] != 3 + n + n * n:
            raise _lib.DimensionMismatch(f"a moment block for n = {n} has {3 + n + n * n} entries, got {block.shape[0]}")
        self.n = int(n)
        self.count = float(block[0])
        self.lp_sum = float(block[1])
        self.lp_sqsum = float(block[2])
        self.score_sum = block[3:3 + n].copy()
        self.outer = block[3 + n:].reshape(n, n, order="F").copy()

    @property
    def fisher(self) -> np.ndarray:
        """``E[g gᵀ]`` (n, n): the Fisher matrix when the samples were drawn from the flow."""
        return self.outer / self.count

    @property
    def mean_score(self) -> np.ndarray:
        return self.score_sum / self.count

    @property
    def score_cov(self) -> np.ndarray:
        m = self.mean_score
        return self.fisher - np.outer(m, m)

    @property
    def entropy(self) -> float:
        """``-E[lp]``: the entropy when the samples were drawn from the flow."""
        return -self.lp_sum / self.count

    @property
    def entropy_stderr(self) -> float:
        mean = self.lp_sum / self.count
        return float(np.sqrt(max(0.0, self.lp_sqsum / self.count - mean * mean) / self.count))

    def __repr__(self):
        return f"ScoreMoments(n={self.n}, count={self.count:g})"


def _check_draws(flow: Flow, theta, n_samples: int, chunk: int):
    """The argument checks of :func:`fisher_information` and :func:`entropy`, before any library call."""
    if not isinstance(theta, tuple) or len(theta) != flow.n:
        raise _lib.DimensionMismatch(f"θ must be a tuple of the flow's n = {flow.n} conditions")
    if int(n_samples) < 0:
        raise _lib.DimensionMismatch("n_samples must be >= 0")
    if int(chunk) < 0:
        raise _lib.DimensionMismatch("chunk must be >= 0 (0: the library's default)")
    if int(chunk) > MAX_CHUNK:
        raise _lib.UnsupportedError("a chunk holds at most 2^24 samples")


def _score_trainer(flow: Flow, state, who: str):
    """(trainer, chain, temporary): ``state``'s trainer, or a temporary one on the flow's chain
    holding the model's current parameters (as :func:`logpdf_grad` makes one)."""
    from .train import Adam, HIPTrainer

    if state is not None:
        return state.trainer, state.trainer.chain, False
    h = flow.hip()
    try:
        h.set_weights(flow.model.layers)
    except _lib.ArgumentError as e:
        raise _lib.ArgumentError(f"{who}: the flow has a live TrainState, pass it as state= ({e})") from e
    return HIPTrainer(h, Adam()), h, True


def _read_block(out, h):
    import torch

    torch.cuda.synchronize(h.device)
    return out.cpu().numpy()


def score_moments(flow: Flow, x, theta=None, state=None) -> ScoreMoments:
    """The moments of :func:`logpdf_grad`'s ``lp`` and ``gθ`` over the points ``x`` (d, dims...),
    reduced on the device (``df_train_score_moments``): only 3 + n + n² doubles reach the host.
    θ (raw) and ``state`` as for :func:`logpdf_grad`."""
    import torch

    th = flow._theta(theta, x)
    tr, h, temporary = _score_trainer(flow, state, "score_moments")
    try:
        xb, thb, dims, batch, _ = h._inputs(x, th, "x")
        out = torch.empty(3 + h.n + h.n * h.n, dtype=torch.float64, device=h.device)
        tr.score_moments(xb, thb, batch, out)
        block = _read_block(out, h)
    finally:
        if temporary:
            tr.close()
    return ScoreMoments(block, h.n)


def fisher_information(flow: Flow, theta: tuple, n_samples: int, chunk: int = 0, rng=None,
                       seed: Optional[int] = None, offset: int = 0, state=None) -> ScoreMoments:
    """The score moments over ``n_samples`` draws of the flow at the ONE raw condition ``theta``
    (a tuple of n values), drawn, differentiated and reduced ``chunk`` samples at a time on the
    device (``df_train_fisher``): ``.fisher`` is ``F(θ) = E_{x~q(x|θ)}[∂θ logq ∂θ logqᵀ]``,
    ``.mean_score`` its Monte-Carlo check (it tends to 0), ``.entropy`` comes along.  Sample s
    is sample s of ``sample(flow, n_samples, theta, seed=seed, offset=offset)``.  ``state`` as
    for :func:`logpdf_grad`."""
    import torch

    _check_draws(flow, theta, n_samples, chunk)
    seed = _draw_seed(rng, seed)
    tr, h, temporary = _score_trainer(flow, state, "fisher_information")
    try:
        out = torch.empty(3 + h.n + h.n * h.n, dtype=torch.float64, device=h.device)
        tr.fisher(_theta_vector(theta, h.device) if h.n > 0 else None, int(n_samples), out, int(chunk), seed,
                  int(offset))
        block = _read_block(out, h)
    finally:
        if temporary:
            tr.close()
    return ScoreMoments(block, h.n)


def entropy(flow: Flow, n_samples: int, theta: tuple = (), chunk: int = 0, rng=None, seed: Optional[int] = None,
            offset: int = 0) -> ScoreMoments:
    """``{count, Σ lp, Σ lp²}`` of ``lp = log q(x | θ)`` over ``n_samples`` draws at the ONE raw
    condition ``theta``, one forward pass per sample and no trainer
    (``df_flow_sample_logpdf_moments``; every chain class): ``.entropy`` is ``H = -E[log q]``,
    ``.entropy_stderr`` its standard error.  The score entries are empty (n = 0 in the result)."""
    import torch

    _check_draws(flow, theta, n_samples, chunk)
    seed = _draw_seed(rng, seed)
    h = flow.hip()
    out = torch.empty(3, dtype=torch.float64, device=h.device)
    h.run_sample_logpdf_moments(_theta_vector(theta, h.device) if h.n > 0 else None, int(n_samples), int(chunk),
                                seed, int(offset), out)
    return ScoreMoments(_read_block(out, h), 0)


def hpd_levels(flow: Flow, x, theta=None, n_draws: int = 1024, chunk: int = 0, rng=None, seed: Optional[int] = None,
               offset: int = 0, return_ranks: bool = False, return_logpdf: bool = False):
    """The credibility levels of the expected-coverage (HPD rank) test, one library call
    (``df_flow_hpd_ranks``; every chain class): for every point ``x[:, j]`` under its condition,
    ``n_draws`` samples of ``q(. | θ_j)`` are drawn on the device and those with a higher density
    than the point are counted there; the level is ``rank / n_draws``, uniform on [0, 1] for a
    calibrated flow (:func:`expected_coverage`).

    ``x`` is (d, dims...); ``theta`` an array (n, dims...) of raw θ or an NTuple used for every
    point (broadcast on the device).  ``n_draws`` is a positive multiple of 4; ``chunk`` (in
    samples, 0: 2²⁰, at most 2²⁴) bounds the workspace and does not change the result within
    one chain-pass kernel family.  Draw k of point j is sample ``j·n_draws + k`` of
    ``sample_logpdf`` at ``(seed, offset)`` with θ repeated per point.

    Returns the float64 levels of shape ``dims`` (numpy); with ``return_ranks`` the int32 ranks
    and with ``return_logpdf`` the points' float32 logpdf follow, in that order.  The count is
    a Float32 ``>``: a point whose own logpdf is NaN (a non-finite or overflowing ``x``) counts
    nothing and gets level 0; ask for the logpdf where the points may be non-finite."""
    import torch

    if len(x.shape) < 1 or int(x.shape[0]) != flow.d:
        raise _lib.DimensionMismatch(f"x must have size ({flow.d}, dims...), got {tuple(x.shape)}")
    dims = tuple(int(v) for v in x.shape[1:])
    bad = AssertionError("dimensions θ must match (n, dims...) with n number of trained parameters")
    if flow.n > 0:
        if theta is None or (isinstance(theta, tuple) and len(theta) != flow.n):
            raise bad
        if not isinstance(theta, tuple) and tuple(theta.shape) != (flow.n,) + dims:
            raise bad
    n_draws = int(n_draws)
    if n_draws <= 0 or n_draws % 4 != 0:
        raise _lib.ArgumentError("n_draws must be a positive multiple of 4 (a Philox counter boundary)")
    if n_draws > MAX_CHUNK:
        raise _lib.UnsupportedError("a point has at most 2^24 draws (n_draws)")
    if int(chunk) < 0:
        raise _lib.DimensionMismatch("chunk must be >= 0 (0: the library's default)")
    if int(chunk) > MAX_CHUNK:
        raise _lib.UnsupportedError("a chunk holds at most 2^24 samples")
    seed = _draw_seed(rng, seed)
    h = flow.hip()
    dev = h.device
    xb, _, _ = as_julia_device(x, flow.d, dev, "x")
    M = int(np.prod(dims)) if dims else 1
    ranks = torch.empty(M, dtype=torch.int32, device=dev)
    lpb = torch.empty(M, dtype=torch.float32, device=dev) if return_logpdf else None
    with torch.cuda.device(dev):
        thb = None
        if flow.n > 0:
            if isinstance(theta, tuple):
                thb = torch.empty(flow.n * M, dtype=torch.float32, device=dev)
                h.run_theta_broadcast(thb, _theta_vector(theta, dev), M)
            else:
                thb, _, _ = as_julia_device(theta, flow.n, dev, "θ")
        if M > 0:
            h.run_hpd_ranks(xb, thb, M, n_draws, int(chunk), seed, int(offset), ranks, lpb)
        torch.cuda.synchronize(dev)
    shape = lambda t: t.cpu().numpy().reshape(dims, order="F")
    r = shape(ranks)
    out = (r.astype(np.float64) / n_draws,)
    if return_ranks:
        out += (r,)
    if return_logpdf:
        out += (shape(lpb),)
    return out if len(out) > 1 else out[0]


def expected_coverage(levels, credibility=None):
    """The expected-coverage curve of credibility levels (:func:`hpd_levels`), on the host:
    ``(c, mean(levels <= c))`` for a grid of credibilities ``c`` (default
    ``linspace(0, 1, 101)``).  A calibrated density gives the diagonal; a curve above it is
    under-confident (too wide), below it over-confident.  Levels are multiples of
    ``1 / n_draws``, so the curve is exact only to O(1 / n_draws).  NaN levels are refused."""
    lv = np.asarray(levels, dtype=np.float64).ravel()
    if np.any(np.isnan(lv)):
        raise _lib.ArgumentError("expected_coverage: NaN levels")
    c = np.linspace(0.0, 1.0, 101) if credibility is None else np.asarray(credibility, dtype=np.float64).ravel()
    if np.any(np.isnan(c)):
        raise _lib.ArgumentError("expected_coverage: NaN credibility")
    if lv.size == 0:
        raise _lib.ArgumentError("expected_coverage: no levels")
    cov = np.searchsorted(np.sort(lv), c, side="right") / lv.size
    return c, cov


# ---------------------------------------------------------------------------
# posterior summaries per condition, reduced on the device (df_pstats.hip)
# ---------------------------------------------------------------------------

class PointStats:
    """What :func:`posterior_stats` returns, as numpy arrays in ``dims`` shape (``order="F"``):
    ``mean`` (d, dims...) and ``cov`` (d, d, dims...) float64 of the ``n_draws`` draws of every
    condition (the covariance with ``n_draws − 1`` in the denominator), ``std`` the square root
    of its diagonal, and ``ranks`` (d, dims...) int32, the SBC ranks ``#{draw[k] < x[k]}`` when
    points were given, else ``None``."""

    def __init__(self, mean, cov, ranks, n_draws: int):
        self.mean, self.cov, self.ranks, self.n_draws = mean, cov, ranks, int(n_draws)

    @property
    def std(self) -> np.ndarray:
        d = self.mean.shape[0]
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.cov[np.arange(d), np.arange(d)])

    def zscore(self, x_true) -> np.ndarray:
        """``(mean − x_true) / std`` per dimension and condition."""
        x_true = np.asarray(x_true, dtype=np.float64)
        if x_true.shape != self.mean.shape:
            raise _lib.DimensionMismatch(f"x_true must have size {self.mean.shape}, got {x_true.shape}")
        return (self.mean - x_true) / self.std

    def __repr__(self):
        return f"PointStats(d={self.mean.shape[0]}, dims={self.mean.shape[1:]}, n_draws={self.n_draws})"


def moments_from_sums(block, d: int, n_draws: int):
    """``(mean (d, M), cov (d, d, M))`` in float64 from the M blocks of ``df_flow_point_stats``'
    ``sums_out`` — the shift ``c``, ``S1 = Σ (v − c)`` and the lower triangle of
    ``S2 = Σ (v − c)(v − c)ᵀ``: ``mean = c + S1/N``, ``cov = (S2 − S1 S1ᵀ/N)/(N − 1)``."""
    S = 2 * d + d * (d + 1) // 2
    blk = np.asarray(block, dtype=np.float64).reshape(-1, S)
    N = float(n_draws)
    c, s1 = blk[:, :d], blk[:, d:2 * d]
    a, b = np.tril_indices(d)                 # row-major lower triangle: index a(a+1)/2 + b
    s2 = np.empty((blk.shape[0], d, d))
    s2[:, a, b] = blk[:, 2 * d:]
    s2[:, b, a] = blk[:, 2 * d:]
    cov = (s2 - s1[:, :, None] * s1[:, None, :] / N) / (N - 1.0)
    return (c + s1 / N).T, np.moveaxis(cov, 0, -1)


def _check_point_draws(flow: Flow, x, theta, n_draws: int, chunk: int, dims):
    """The argument checks of :func:`posterior_stats` and :func:`sbc_ranks` (those of
    :func:`hpd_levels`), before any library call → ``dims``."""
    if x is not None:
        if len(x.shape) < 1 or int(x.shape[0]) != flow.d:
            raise _lib.DimensionMismatch(f"x must have size ({flow.d}, dims...), got {tuple(x.shape)}")
        xdims = tuple(int(v) for v in x.shape[1:])
        if dims is not None and tuple(int(v) for v in dims) != xdims:
            raise _lib.DimensionMismatch(f"dims = {tuple(dims)} does not match x of size {tuple(x.shape)}")
        dims = xdims
    bad = AssertionError("dimensions θ must match (n, dims...) with n number of trained parameters")
    if flow.n > 0:
        if theta is None or (isinstance(theta, tuple) and len(theta) != flow.n):
            raise bad
        if not isinstance(theta, tuple):
            if len(theta.shape) < 1 or int(theta.shape[0]) != flow.n:
                raise bad
            tdims = tuple(int(v) for v in theta.shape[1:])
            if dims is not None and tuple(int(v) for v in dims) != tdims:
                raise bad
            dims = tdims
    if dims is None:
        raise _lib.ArgumentError("an NTuple θ or an unconditional flow needs the points x or dims=")
    dims = tuple(int(v) for v in dims)
    n_draws = int(n_draws)
    if n_draws <= 0 or n_draws % 4 != 0:
        raise _lib.ArgumentError("n_draws must be a positive multiple of 4 (a Philox counter boundary)")
    if n_draws > MAX_CHUNK:
        raise _lib.UnsupportedError("a point has at most 2^24 draws (n_draws)")
    if int(chunk) < 0:
        raise _lib.DimensionMismatch("chunk must be >= 0 (0: the library's default)")
    if int(chunk) > MAX_CHUNK:
        raise _lib.UnsupportedError("a chunk holds at most 2^24 samples")
    return dims


def _point_stats(flow: Flow, x, theta, n_draws, chunk, rng, seed, offset, dims, want_sums: bool):
    """One ``df_flow_point_stats`` call → (ranks (d, M) int32 or None, sums (M, S) or None, dims)."""
    import torch

    dims = _check_point_draws(flow, x, theta, n_draws, chunk, dims)
    seed = _draw_seed(rng, seed)
    h = flow.hip()
    dev, d = h.device, flow.d
    M = int(np.prod(dims)) if dims else 1
    xb = as_julia_device(x, d, dev, "x")[0] if x is not None else None
    ranks = torch.empty(d * M, dtype=torch.int32, device=dev) if x is not None else None
    S = 2 * d + d * (d + 1) // 2
    sums = torch.empty(M * S, dtype=torch.float64, device=dev) if want_sums else None
    with torch.cuda.device(dev):
        thb = None
        if flow.n > 0:
            if isinstance(theta, tuple):
                thb = torch.empty(flow.n * M, dtype=torch.float32, device=dev)
                h.run_theta_broadcast(thb, _theta_vector(theta, dev), M)
            else:
                thb, _, _ = as_julia_device(theta, flow.n, dev, "θ")
        if M > 0:
            h.run_point_stats(xb, thb, M, int(n_draws), int(chunk), seed, int(offset), ranks, sums)
        torch.cuda.synchronize(dev)
    r = ranks.cpu().numpy().reshape(M, d).T if ranks is not None else None
    return r, (sums.cpu().numpy().reshape(M, S) if want_sums else None), dims


def posterior_stats(flow: Flow, theta=None, n_draws: int = 1024, x=None, chunk: int = 0, rng=None,
                    seed: Optional[int] = None, offset: int = 0, dims=None) -> PointStats:
    """The mean and covariance of ``n_draws`` samples of ``q(. | θ_j)`` for every condition, one
    library call (``df_flow_point_stats``; every chain class): the draws are made and reduced on
    the device, ``d + d(d+1)/2`` fp64 sums and a shift per condition reach the host.  With the
    points ``x`` (d, dims...) the SBC ranks of :func:`sbc_ranks` come along in ``.ranks``.

    ``theta`` is an array (n, dims...) of raw θ, or an NTuple used for every point (broadcast on
    the device), which then needs ``x`` or ``dims=`` for the shape; so does an unconditional
    flow.  ``n_draws``, ``chunk``, ``seed``, ``offset`` as for :func:`hpd_levels`: draw k of
    point j is sample ``j·n_draws + k`` of ``sample`` at ``(seed, offset)`` with θ repeated per
    point, and its base normal is the one :func:`hpd_levels` uses at the same ``(seed, offset)``."""
    r, blk, dims = _point_stats(flow, x, theta, n_draws, chunk, rng, seed, offset, dims, True)
    d = flow.d
    mean, cov = moments_from_sums(blk, d, int(n_draws))
    return PointStats(np.asfortranarray(mean).reshape((d,) + dims, order="F"),
                      np.asfortranarray(cov).reshape((d, d) + dims, order="F"),
                      np.asfortranarray(r).reshape((d,) + dims, order="F") if r is not None else None, int(n_draws))


def sbc_ranks(flow: Flow, x, theta=None, n_draws: int = 1024, chunk: int = 0, rng=None, seed: Optional[int] = None,
              offset: int = 0) -> np.ndarray:
    """The simulation-based-calibration ranks, one library call (``df_flow_point_stats``, its
    ranks-only kernel): for every held-out pair ``(x[:, j], θ_j)`` and dimension k the number of
    ``n_draws`` samples of ``q(. | θ_j)`` whose coordinate k lies below ``x[k, j]`` (a Float32
    ``<``: a NaN coordinate gives rank 0), as int32 (d, dims...).  Uniform on ``{0 .. n_draws}``
    for a calibrated flow (:func:`sbc_histogram`).  Arguments as for :func:`posterior_stats`."""
    if x is None:
        raise _lib.DimensionMismatch(f"x must have size ({flow.d}, dims...), got None")
    r, _, dims = _point_stats(flow, x, theta, n_draws, chunk, rng, seed, offset, None, False)
    return np.asfortranarray(r).reshape((flow.d,) + dims, order="F")


def sbc_histogram(ranks, n_draws: int, bins: int) -> np.ndarray:
    """The counts of SBC ranks (d, dims...) per dimension in ``bins`` equal groups of the
    ``n_draws + 1`` possible values, on the host → int64 (d, bins); flat for a calibrated flow.
    ``bins`` must divide ``n_draws + 1``."""
    n_draws, bins = int(n_draws), int(bins)
    if bins <= 0 or (n_draws + 1) % bins != 0:
        raise _lib.ArgumentError(f"bins must divide n_draws + 1 = {n_draws + 1}")
    r = np.asarray(ranks)
    if r.ndim < 1 or not np.issubdtype(r.dtype, np.integer):
        raise _lib.ArgumentError("ranks must be an integer array (d, dims...)")
    r = r.reshape(r.shape[0], -1)
    if r.size and (r.min() < 0 or r.max() > n_draws):
        raise _lib.ArgumentError(f"ranks outside 0 .. n_draws = {n_draws}")
    width = (n_draws + 1) // bins
    return np.stack([np.bincount(row // width, minlength=bins) for row in r]).astype(np.int64).reshape(r.shape[0], bins)


# ---------------------------------------------------------------------------
# posterior quantiles per condition and dimension, selected on the device (df_quant.hip)
# ---------------------------------------------------------------------------

QUANT_MAX_ORDERS = 32          # DF_QUANT_MAX_ORDERS


def quantile_orders(probs, n_draws: int):
    """The order statistics behind the quantiles ``probs`` of ``n_draws`` draws under the
    ``linear`` (type 7) rule of numpy and of Julia's ``Statistics.quantile``: ``h = p·(N − 1)``,
    ``j = floor(h)``, ``g = h − j``, quantile ``= v[j] + (v[min(j + 1, N − 1)] − v[j])·g`` of the
    sorted draws ``v`` → ``(orders, lo_idx, hi_idx, frac)``: ``orders`` the sorted unique int32
    set of every ``j`` and ``min(j + 1, N − 1)``, ``lo_idx`` / ``hi_idx`` the positions of the two
    in ``orders`` and ``frac`` the float64 ``g``, one per probability.  No library call."""
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
    N = int(n_draws)
    if N <= 0:
        raise _lib.ArgumentError("n_draws must be positive")
    if p.size == 0:
        raise _lib.ArgumentError("no probabilities")
    if not np.all((p >= 0.0) & (p <= 1.0)):            # a NaN fails both comparisons
        raise _lib.ArgumentError("probabilities must lie in [0, 1]")
    h = p * (N - 1)
    j = np.minimum(np.floor(h).astype(np.int64), N - 1)
    frac = h - j
    hi = np.minimum(j + 1, N - 1)
    orders = np.unique(np.concatenate([j, hi]))
    if orders.size > QUANT_MAX_ORDERS:
        raise _lib.ArgumentError(f"{orders.size} order statistics needed, at most {QUANT_MAX_ORDERS} in one call")
    return orders.astype(np.int32), np.searchsorted(orders, j), np.searchsorted(orders, hi), frac


def _check_orders(orders, n_draws: int):
    o = np.atleast_1d(np.asarray(orders))
    if o.ndim != 1 or o.size == 0 or not np.issubdtype(o.dtype, np.integer):
        raise _lib.ArgumentError("orders must be a non-empty vector of integers")
    if o.size > QUANT_MAX_ORDERS:
        raise _lib.UnsupportedError(f"at most {QUANT_MAX_ORDERS} orders in one call")
    if o.min() < 0 or o.max() >= n_draws:
        raise _lib.ArgumentError(f"orders must lie in [0, n_draws = {n_draws})")
    return [int(v) for v in o]


def order_statistics(draws, orders, device=None):
    """The order statistics ``orders`` (0-based integers in ``[0, N)``, any order, repeats
    allowed, at most 32) of every dimension of every point, selected on the device
    (``df_order_statistics``) → float32 ``(M, d, Q)``, a numpy array for numpy draws and a
    device tensor otherwise.  ``draws`` is a numpy ``(M, N, d)`` Float32 array or a device
    tensor of that shape in C order (the layout of ``draws_out``: draw j of point i at
    ``d·(i·N + j)``); ``N`` a multiple of 4, ``d <= 64``.  The order is IEEE totalOrder
    (−NaN < −inf < ... < −0 < +0 < ... < +inf < +NaN); a result is one of the draws, bit for bit."""
    import torch

    from .hip import run_order_statistics

    was_np = not isinstance(draws, torch.Tensor)
    if was_np:
        draws = np.asarray(draws)
        if draws.dtype != np.float32:
            raise _lib.ArgumentError(f"draws must be Float32 (got {draws.dtype})")
    elif draws.dtype != torch.float32:
        raise _lib.ArgumentError(f"draws must be Float32 (got {draws.dtype})")
    if len(draws.shape) != 3:
        raise _lib.DimensionMismatch(f"draws must have size (M, N, d), got {tuple(draws.shape)}")
    M, N, d = (int(v) for v in draws.shape)
    if not 1 <= d <= 64:
        raise _lib.ArgumentError("d must be in 1 .. 64")
    if N <= 0 or N % 4 != 0:
        raise _lib.ArgumentError("n_draws must be a positive multiple of 4")
    if N > MAX_CHUNK:
        raise _lib.UnsupportedError("a point has at most 2^24 draws (n_draws)")
    o = _check_orders(orders, N)
    if was_np:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        xs = torch.from_numpy(np.ascontiguousarray(draws)).to(dev)
    else:
        xs = draws.contiguous()
        if xs.device.type != "cuda":
            xs = xs.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
        if xs.data_ptr() % 16 != 0:
            xs = xs.clone()
    out = torch.empty((M, d, len(o)), dtype=torch.float32, device=xs.device)
    if M > 0:
        run_order_statistics(xs, d, M, N, o, out)
    if was_np:
        torch.cuda.synchronize(xs.device)
        return out.cpu().numpy()
    return out


def _point_quantiles(flow: Flow, theta, probs, n_draws, x, chunk, rng, seed, offset, dims, want_sums, want_draws):
    """One ``df_flow_point_quantiles`` call → (quantiles (P, d, M) float64, ranks (d, M) or None,
    sums (M, S) or None, draws (M, N, d) float32 or None, dims)."""
    import torch

    dims = _check_point_draws(flow, x, theta, n_draws, chunk, dims)
    N = int(n_draws)
    orders, lo_i, hi_i, frac = quantile_orders(probs, N)
    seed = _draw_seed(rng, seed)
    h = flow.hip()
    dev, d = h.device, flow.d
    M = int(np.prod(dims)) if dims else 1
    Q = int(orders.size)
    xb = as_julia_device(x, d, dev, "x")[0] if x is not None else None
    quant = torch.empty(M * d * Q, dtype=torch.float32, device=dev)
    ranks = torch.empty(d * M, dtype=torch.int32, device=dev) if x is not None and want_sums else None
    S = 2 * d + d * (d + 1) // 2
    sums = torch.empty(M * S, dtype=torch.float64, device=dev) if want_sums else None
    draws = torch.empty(M * N * d, dtype=torch.float32, device=dev) if want_draws else None
    with torch.cuda.device(dev):
        thb = None
        if flow.n > 0:
            if isinstance(theta, tuple):
                thb = torch.empty(flow.n * M, dtype=torch.float32, device=dev)
                h.run_theta_broadcast(thb, _theta_vector(theta, dev), M)
            else:
                thb, _, _ = as_julia_device(theta, flow.n, dev, "θ")
        if M > 0:
            h.run_point_quantiles(xb if ranks is not None else None, thb, M, N, int(chunk), seed, int(offset),
                                  orders, quant, ranks, sums, draws)
        torch.cuda.synchronize(dev)
    v = quant.cpu().numpy().reshape(M, d, Q).astype(np.float64)
    lo, hi = v[:, :, lo_i], v[:, :, hi_i]                     # (M, d, P)
    with np.errstate(invalid="ignore"):
        qv = lo + (hi - lo) * frac
    qv = np.where((frac == 0.0) | (lo == hi), lo, qv)         # an order statistic itself, also when infinite
    r = ranks.cpu().numpy().reshape(M, d).T if ranks is not None else None
    return (np.ascontiguousarray(qv.transpose(2, 1, 0)), r, sums.cpu().numpy().reshape(M, S) if want_sums else None,
            draws.cpu().numpy().reshape(M, N, d) if want_draws else None, dims)


def posterior_quantiles(flow: Flow, theta=None, probs=(0.16, 0.5, 0.84), n_draws: int = 1024, x=None, chunk: int = 0,
                        rng=None, seed: Optional[int] = None, offset: int = 0, return_stats: bool = False,
                        dims=None, return_draws: bool = False):
    """The quantiles ``probs`` of every dimension of ``n_draws`` samples of ``q(. | θ_j)`` for
    every condition, one library call (``df_flow_point_quantiles``; every chain class): the draws
    are made on the device, the order statistics that the quantiles need (:func:`quantile_orders`,
    at most 32) are selected there exactly, and ``d · len(orders)`` floats per condition reach the
    host → float64 ``(len(probs), d, dims...)``, ``lo + (hi − lo)·g`` of the two order statistics
    in float64: ``np.quantile`` (``linear``) of the draws.

    With ``return_stats=True`` the :class:`PointStats` of the same draws come along — the value
    is ``(quantiles, stats)`` — with the SBC ranks when the points ``x`` are given; with
    ``return_draws=True`` the draws themselves, numpy ``(M, n_draws, d)``, are appended.  The
    other arguments, their checks and the draws are those of :func:`posterior_stats` at the same
    ``(seed, offset)``."""
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    qv, r, blk, draws, dims = _point_quantiles(flow, theta, probs, n_draws, x, chunk, rng, seed, offset, dims,
                                               bool(return_stats), bool(return_draws))
    d = flow.d
    out = np.stack([np.asfortranarray(q).reshape((d,) + dims, order="F") for q in qv])
    res = [out]
    if return_stats:
        mean, cov = moments_from_sums(blk, d, int(n_draws))
        res.append(PointStats(np.asfortranarray(mean).reshape((d,) + dims, order="F"),
                              np.asfortranarray(cov).reshape((d, d) + dims, order="F"),
                              np.asfortranarray(r).reshape((d,) + dims, order="F") if r is not None else None,
                              int(n_draws)))
    if return_draws:
        res.append(draws)
    return res[0] if len(res) == 1 else tuple(res)


def credible_intervals(flow: Flow, theta=None, level: float = 0.68, n_draws: int = 1024, x=None, chunk: int = 0,
                       rng=None, seed: Optional[int] = None, offset: int = 0, dims=None):
    """The equal-tailed credible interval of every dimension and condition →
    ``(lower, median, upper)``, each float64 ``(d, dims...)``: :func:`posterior_quantiles` at
    ``probs = ((1 − level)/2, 0.5, (1 + level)/2)``; ``0 < level < 1``."""
    level = float(level)
    if not 0.0 < level < 1.0:                                 # a NaN fails both comparisons
        raise _lib.ArgumentError("level must lie in (0, 1)")
    q = posterior_quantiles(flow, theta, ((1.0 - level) / 2, 0.5, (1.0 + level) / 2), n_draws, x, chunk, rng, seed,
                            offset, False, dims)
    return q[0], q[1], q[2]


# ---------------------------------------------------------------------------
# posterior histograms per condition: 1-D and 2-D marginal counts on the device (df_hist.hip)
# ---------------------------------------------------------------------------

HIST_MAX_BINS = 128            # DF_HIST_MAX_BINS
HIST_MAX_TABLES = 2080         # DF_HIST_MAX_TABLES
HIST_SPLIT_DRAWS = 2048        # DF_HIST_SPLIT_DRAWS


def histogram_edges(spec, d: int):
    """The per-dimension bin edges of the histogram calls → ``(edges, bins)``: ``edges`` a list of
    d Float32 vectors (``None`` for a dimension without bins) and ``bins`` the d int32 bin counts
    (0 there).  ``spec`` holds one entry per dimension: ``None``, a 1-D increasing array of 2 to
    129 edges, or a tuple ``(lo, hi, nbins)`` with an integer ``nbins`` — ``np.linspace(lo, hi,
    nbins + 1)`` in float64, rounded to Float32.  Edges must be free of NaN and strictly
    increasing as Float32 (infinite outer edges are allowed).  No library call."""
    d = int(d)
    spec = list(spec)
    if len(spec) != d:
        raise _lib.DimensionMismatch(f"edges must hold d = {d} entries (None, an array or (lo, hi, nbins)), got {len(spec)}")
    edges, bins = [], np.zeros(d, np.int32)
    for k, e in enumerate(spec):
        if e is None:
            edges.append(None)
            continue
        if isinstance(e, tuple) and len(e) == 3 and isinstance(e[2], (int, np.integer)) and not isinstance(e[2], bool):
            lo, hi, nb = float(e[0]), float(e[1]), int(e[2])
            if nb < 1 or nb > HIST_MAX_BINS:
                raise _lib.ArgumentError(f"edges of dimension {k}: nbins = {nb} is outside 1 .. {HIST_MAX_BINS}")
            e = np.linspace(lo, hi, nb + 1, dtype=np.float64)
        if hasattr(e, "detach"):
            e = e.detach().cpu().numpy()
        with np.errstate(over="ignore"):
            v = np.asarray(e, dtype=np.float64).astype(np.float32)
        if v.ndim != 1:
            raise _lib.ArgumentError(f"edges of dimension {k} must be a vector, got size {v.shape}")
        if v.size < 2:
            raise _lib.ArgumentError(f"edges of dimension {k}: fewer than 2 edges")
        if v.size > HIST_MAX_BINS + 1:
            raise _lib.ArgumentError(f"edges of dimension {k}: more than {HIST_MAX_BINS + 1} edges")
        if np.any(np.isnan(v)):
            raise _lib.ArgumentError(f"edges of dimension {k} hold NaN")
        if not np.all(v[1:] > v[:-1]):
            raise _lib.ArgumentError(f"edges of dimension {k} are not strictly increasing as Float32")
        edges.append(v)
        bins[k] = v.size - 1
    return edges, bins


def _histogram_requests(keep, bins):
    """``keep`` → sorted, distinct tuples ``(a,)`` / ``(a, b)`` with a < b, 1-D tables first
    (the order of :func:`pdf_marginals`); ``None``: every dimension with bins, then every pair."""
    d = len(bins)
    if keep is None:
        xs = [k for k in range(d) if bins[k] > 0]
        keep = [(a,) for a in xs] + [(a, b) for i, a in enumerate(xs) for b in xs[i + 1:]]
    out = set()
    for K in keep:
        K = (int(K),) if np.ndim(K) == 0 else tuple(int(v) for v in K)
        if len(K) > 2:
            raise _lib.UnsupportedError(f"a histogram keeps at most two dimensions, got {K}")
        if len(K) == 0 or len(set(K)) != len(K) or any(v < 0 or v >= d for v in K):
            raise _lib.ArgumentError(f"kept dimensions must be one or two distinct numbers in [0, {d}), got {K}")
        if any(bins[v] == 0 for v in K):
            raise _lib.ArgumentError(f"keep {K} names a dimension without edges")
        out.add(tuple(sorted(K)))
    out = sorted(out, key=lambda K: (len(K), K))
    if not out:
        raise _lib.ArgumentError("no histogram tables: keep is empty or no dimension has edges")
    if len(out) > HIST_MAX_TABLES:
        raise _lib.UnsupportedError(f"at most {HIST_MAX_TABLES} histogram tables per call, got {len(out)}")
    return out


def _histogram_tables(flat, M: int, reqs, bins):
    """The (M, T) int32 blocks (numpy or tensor) → ``{K: (M, L_a) or (M, L_a, L_b)}`` views."""
    res, at = {}, 0
    for K in reqs:
        if len(K) == 1:
            size = int(bins[K[0]])
            res[K] = flat[:, at:at + size]
        else:
            la, lb = int(bins[K[0]]), int(bins[K[1]])
            size = la * lb
            t = flat[:, at:at + size].reshape(M, lb, la)          # the lower dimension runs fastest
            res[K] = t.transpose(0, 2, 1) if isinstance(t, np.ndarray) else t.permute(0, 2, 1)
        at += size
    return res


def draw_histograms(draws, edges, keep=None, device=None):
    """The 1-D and 2-D marginal histograms of every point's draws, counted on the device
    (``df_draw_histograms``) → ``{(a,): (M, L_a), (a, b): (M, L_a, L_b)}`` in int32, keys sorted
    (1-D tables first), the shape convention of ``np.histogram2d`` and of :func:`pdf_marginals`;
    numpy arrays for numpy draws and device tensors otherwise.  ``draws`` is a numpy
    ``(M, N, d)`` Float32 array or a device tensor of that shape in C order (the layout of
    ``draws_out``); ``N`` a multiple of 4, ``d <= 64``.  ``edges``: the per-dimension entries of
    :func:`histogram_edges`.  ``keep``: the tables wanted, each one dimension or a pair (sorted,
    duplicates merged); ``None`` is the corner plot, every dimension with edges and every pair of
    them.  The counts are ``np.histogram`` / ``np.histogram2d`` of the same Float32 draws bit for
    bit: bin j holds ``e_j <= v < e_{j+1}``, the last bin also ``v == e_L``; draws outside, and
    NaN, are counted nowhere in the tables that keep the dimension."""
    import torch

    from .hip import run_draw_histograms

    was_np = not isinstance(draws, torch.Tensor)
    if was_np:
        draws = np.asarray(draws)
        if draws.dtype != np.float32:
            raise _lib.ArgumentError(f"draws must be Float32 (got {draws.dtype})")
    elif draws.dtype != torch.float32:
        raise _lib.ArgumentError(f"draws must be Float32 (got {draws.dtype})")
    if len(draws.shape) != 3:
        raise _lib.DimensionMismatch(f"draws must have size (M, N, d), got {tuple(draws.shape)}")
    M, N, d = (int(v) for v in draws.shape)
    if not 1 <= d <= 64:
        raise _lib.ArgumentError("d must be in 1 .. 64")
    if N <= 0 or N % 4 != 0:
        raise _lib.ArgumentError("n_draws must be a positive multiple of 4")
    if N > MAX_CHUNK:
        raise _lib.UnsupportedError("a point has at most 2^24 draws (n_draws)")
    ev, bins = histogram_edges(edges, d)
    reqs = _histogram_requests(keep, bins)
    T = sum(int(np.prod([bins[k] for k in K])) for K in reqs)
    if was_np:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        xs = torch.from_numpy(np.ascontiguousarray(draws)).to(dev)
    else:
        xs = draws.contiguous()
        if xs.device.type != "cuda":
            xs = xs.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)
        if xs.data_ptr() % 16 != 0:
            xs = xs.clone()
    eb = torch.from_numpy(np.concatenate([v for v in ev if v is not None])).to(xs.device)
    out = torch.empty((M, T), dtype=torch.int32, device=xs.device)
    if M > 0:
        run_draw_histograms(xs, d, M, N, eb, bins, reqs, out)
    if was_np:
        torch.cuda.synchronize(xs.device)
        return _histogram_tables(out.cpu().numpy(), M, reqs, bins)
    return _histogram_tables(out, M, reqs, bins)


class PointHistograms:
    """What :func:`posterior_histograms` returns: ``counts``, the dict
    ``{(a,): (M, L_a), (a, b): (M, L_a, L_b)}`` of int32 numpy arrays over the M = prod(dims)
    conditions (flat, first of ``dims`` fastest), ``edges`` (d Float32 vectors, ``None`` for a
    dimension without bins), ``n_draws`` and ``dims``."""

    def __init__(self, counts, edges, n_draws: int, dims=()):
        self.counts, self.edges, self.n_draws, self.dims = counts, edges, int(n_draws), tuple(dims)

    @staticmethod
    def _key(K):
        return (int(K),) if np.ndim(K) == 0 else tuple(int(v) for v in K)

    def inside(self, K) -> np.ndarray:
        """The number of draws inside the table's range per condition, int64 (M,): its sum."""
        c = self.counts[self._key(K)]
        return c.reshape(c.shape[0], -1).sum(axis=1, dtype=np.int64)

    def density(self, K) -> np.ndarray:
        """``counts / (n_draws · bin width)`` (1-D) or ``/ (n_draws · bin area)`` (2-D) in
        float64: it integrates to the inside fraction ``inside(K) / n_draws``.  A bin with an
        infinite edge has density 0."""
        K = self._key(K)
        w = np.diff(self.edges[K[0]].astype(np.float64))
        if len(K) == 2:
            w = w[:, None] * np.diff(self.edges[K[1]].astype(np.float64))[None, :]
        return self.counts[K].astype(np.float64) / (float(self.n_draws) * w)

    def pooled(self, K) -> np.ndarray:
        """The table summed over the conditions, int64."""
        return self.counts[self._key(K)].sum(axis=0, dtype=np.int64)

    def __repr__(self):
        return f"PointHistograms(tables={len(self.counts)}, dims={self.dims}, n_draws={self.n_draws})"


def posterior_histograms(flow: Flow, theta=None, edges=None, keep=None, n_draws: int = 1024, chunk: int = 0,
                         rng=None, seed: Optional[int] = None, offset: int = 0, dims=None,
                         return_draws: bool = False):
    """The 1-D and 2-D marginal histograms of ``n_draws`` samples of ``q(. | θ_j)`` for every
    condition — the corner plot — one library call (``df_flow_point_histograms``; every chain
    class): the draws are made and counted on the device, only the integer tables reach the host
    → :class:`PointHistograms`.  ``edges`` and ``keep`` as for :func:`draw_histograms`; ``theta``,
    ``dims``, ``n_draws``, ``chunk`` and the seed arguments, their checks and the draws are those
    of :func:`posterior_quantiles` at the same ``(seed, offset)``.  With ``return_draws=True`` the
    value is ``(histograms, draws)``, the draws numpy ``(M, n_draws, d)``.  The counts are exact
    and bitwise reproducible, whatever the chunk."""
    import torch

    dims = _check_point_draws(flow, None, theta, n_draws, chunk, dims)
    if edges is None:
        raise _lib.ArgumentError("posterior_histograms needs edges: one entry per dimension")
    d, N = flow.d, int(n_draws)
    ev, bins = histogram_edges(edges, d)
    reqs = _histogram_requests(keep, bins)
    T = sum(int(np.prod([bins[k] for k in K])) for K in reqs)
    seed = _draw_seed(rng, seed)
    h = flow.hip()
    dev = h.device
    M = int(np.prod(dims)) if dims else 1
    counts = torch.empty((M, T), dtype=torch.int32, device=dev)
    draws = torch.empty(M * N * d, dtype=torch.float32, device=dev) if return_draws else None
    eb = torch.from_numpy(np.concatenate([v for v in ev if v is not None])).to(dev)
    with torch.cuda.device(dev):
        thb = None
        if flow.n > 0:
            if isinstance(theta, tuple):
                thb = torch.empty(flow.n * M, dtype=torch.float32, device=dev)
                h.run_theta_broadcast(thb, _theta_vector(theta, dev), M)
            else:
                thb, _, _ = as_julia_device(theta, flow.n, dev, "θ")
        if M > 0:
            h.run_point_histograms(thb, M, N, int(chunk), seed, int(offset), eb, bins, reqs, counts, draws)
        torch.cuda.synchronize(dev)
    res = PointHistograms(_histogram_tables(counts.cpu().numpy(), M, reqs, bins), ev, N, dims)
    if return_draws:
        return res, draws.cpu().numpy().reshape(M, N, d)
    return res


# ---------------------------------------------------------------------------
# importance weights: evidence, effective sample size, weighted moments (df_iw.hip)
# ---------------------------------------------------------------------------

def posterior_draws(flow: Flow, theta=None, n_draws: int = 1024, dims=None, rng=None, seed: Optional[int] = None,
                    offset: int = 0, return_logpdf: bool = True, as_tensor: bool = False):
    """``n_draws`` samples of ``q(. | θ_i)`` for every condition together with their ``log q``, one
    library call (``df_flow_sample_logpdf`` with θ row i repeated over its draws) → ``(draws, logq)``
    of shapes ``(M, n_draws, d)`` and ``(M, n_draws)`` in Float32, M = prod(dims) (flat, first of
    ``dims`` fastest): the layout :func:`weighted_stats`, :func:`order_statistics` and
    :func:`draw_histograms` take.  Draw k of point i is sample ``i·n_draws + k`` of that call: its
    ``log q`` is bitwise the ``draws_logpdf_out`` of ``df_flow_hpd_ranks`` at the same
    ``(seed, offset)`` within one chain-pass kernel family.  ``theta``, ``dims``, ``n_draws`` and
    the seed arguments and their checks are those of :func:`posterior_stats`.  With
    ``return_logpdf=False`` the value is the draws alone; with ``as_tensor=True`` both stay on the
    device (nothing synchronises)."""
    import torch

    dims = _check_point_draws(flow, None, theta, n_draws, 0, dims)
    N = int(n_draws)
    seed = _draw_seed(rng, seed)
    h = flow.hip()
    dev, d, n = h.device, flow.d, flow.n
    M = int(np.prod(dims)) if dims else 1
    draws = torch.empty((M, N, d), dtype=torch.float32, device=dev)
    lq = torch.empty((M, N), dtype=torch.float32, device=dev) if return_logpdf else None
    with torch.cuda.device(dev):
        th_rep = None
        if n > 0:
            if isinstance(theta, tuple):
                th_rep = torch.empty(n * M * N, dtype=torch.float32, device=dev)
                if M > 0:
                    h.run_theta_broadcast(th_rep, _theta_vector(theta, dev), M * N)
            else:
                thb, _, _ = as_julia_device(theta, n, dev, "θ")
                th_rep = thb.view(M, n).repeat_interleave(N, dim=0).reshape(-1)
        if M > 0:
            h.run_sample_logpdf(draws.view(-1), lq.view(-1) if return_logpdf else None, th_rep, False, M * N, seed,
                                int(offset))
        if not as_tensor:
            torch.cuda.synchronize(dev)
    if not as_tensor:
        draws = draws.cpu().numpy()
        lq = lq.cpu().numpy() if return_logpdf else None
    return (draws, lq) if return_logpdf else draws


def _check_mn(a, name: str, shape=None):
    """The host checks of an ``(M, N)`` Float32 array (numpy or tensor), no library call →
    ``(M, N)``.  ``shape``: the size it must have."""
    import torch

    is_t = isinstance(a, torch.Tensor)
    if not is_t:
        a = np.asarray(a)
    if a.dtype != (torch.float32 if is_t else np.float32):
        raise _lib.ArgumentError(f"{name} must be Float32 (got {a.dtype})")
    if len(a.shape) != 2:
        raise _lib.DimensionMismatch(f"{name} must have size (M, N), got {tuple(a.shape)}")
    M, N = (int(v) for v in a.shape)
    if shape is not None and (M, N) != tuple(shape):
        raise _lib.DimensionMismatch(f"{name} must have size {tuple(shape)}, got {(M, N)}")
    if N <= 0 or N % 4 != 0:
        raise _lib.ArgumentError("n_draws must be a positive multiple of 4")
    if N > MAX_CHUNK:
        raise _lib.UnsupportedError("a point has at most 2^24 draws (n_draws)")
    return M, N


def _device_rows(a, dev):
    """A checked array as a C-contiguous, 16-byte aligned float32 device tensor of its shape."""
    import torch

    if not isinstance(a, torch.Tensor):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = a.contiguous()
    if t.device.type != "cuda":
        t = t.to(dev)
    return t.clone() if t.data_ptr() % 16 != 0 else t


def _default_device(*arrays):
    import torch

    for a in arrays:
        if isinstance(a, torch.Tensor) and a.device.type == "cuda":
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


class ImportanceWeights:
    """What :func:`importance_weights` returns for M points of N draws: ``w`` ``(M, N)`` Float32, the
    stabilised weights ``exp(logw − max)`` (numpy for numpy input, a device tensor otherwise; the
    largest of a point is 1), and float64 numpy vectors of length M: ``log_max``,
    ``sum_w`` = W1 = Σ w, ``sum_w2`` = W2 = Σ w², ``n_positive`` (int64) the number of draws with
    a weight above 0, and from them ``log_evidence = log_max + log(W1/N)``, its standard error
    ``log_evidence_stderr = sqrt((N·W2/W1² − 1)/(N − 1))`` (the delta method),
    ``ess = W1²/W2`` and ``efficiency = ess/N``."""

    def __init__(self, w, stats, n_draws: int, device_w=None):
        st = np.asarray(stats, dtype=np.float64).reshape(-1, 4)
        self.w, self.n_draws, self._device_w = w, int(n_draws), device_w
        self.log_max, self.sum_w, self.sum_w2 = st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy()
        with np.errstate(invalid="ignore"):
            self.n_positive = st[:, 3].astype(np.int64)

    @property
    def log_evidence(self) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.log_max + np.log(self.sum_w / float(self.n_draws))

    @property
    def ess(self) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.sum_w * self.sum_w / self.sum_w2

    @property
    def efficiency(self) -> np.ndarray:
        return self.ess / float(self.n_draws)

    @property
    def log_evidence_stderr(self) -> np.ndarray:
        N = float(self.n_draws)
        with np.errstate(divide="ignore", invalid="ignore"):
            var = (N * self.sum_w2 / (self.sum_w * self.sum_w) - 1.0) / (N - 1.0)
            return np.sqrt(np.where(var < 0.0, 0.0, var))        # (a rounding below 0 at equal weights)

    def normalized(self):
        """``w / Σ w`` per point in float64, shape ``(M, N)``: weights that sum to 1."""
        if isinstance(self.w, np.ndarray):
            return self.w.astype(np.float64) / self.sum_w[:, None]
        import torch

        return self.w.double() / torch.from_numpy(self.sum_w).to(self.w.device)[:, None]

    def __repr__(self):
        return f"ImportanceWeights(points={self.sum_w.shape[0]}, n_draws={self.n_draws})"


def importance_weights(log_target, log_proposal=None, device=None) -> ImportanceWeights:
    """The importance weights of per-point draws, on the device (``df_importance_weights``):
    ``logw = log_target − log_proposal`` (one Float32 subtraction; ``log_proposal=None``:
    ``log_target`` holds the log-weights themselves), stabilised per point with its largest
    non-NaN value, exponentiated and summed in fp64 in a fixed order → :class:`ImportanceWeights`.
    Both arguments are ``(M, N)`` Float32, numpy arrays or device tensors — the ``log q`` of
    :func:`posterior_draws` and the unnormalised log-posterior at its draws; ``N`` a multiple of 4.
    Dtype and shape are checked before the library is touched; the values are not (``−inf`` gives
    weight 0, a NaN or ``+inf``, or a point of ``−inf`` alone, NaN sums for that point only)."""
    import torch

    from .hip import run_importance_weights

    M, N = _check_mn(log_target, "log_target")
    if log_proposal is not None:
        _check_mn(log_proposal, "log_proposal", (M, N))
    was_np = not isinstance(log_target, torch.Tensor)
    dev = torch.device(device) if device is not None else _default_device(log_target, log_proposal)
    lw = _device_rows(log_target, dev)
    if log_proposal is not None:
        lw = lw - _device_rows(log_proposal, dev)
    w = torch.empty((M, N), dtype=torch.float32, device=dev)
    stats = torch.empty((M, 4), dtype=torch.float64, device=dev)
    if M > 0:
        run_importance_weights(lw, M, N, w, stats)
    torch.cuda.synchronize(dev)
    return ImportanceWeights(w.cpu().numpy() if was_np else w, stats.cpu().numpy(), N, w)


class WeightedPointStats:
    """What :func:`weighted_stats` returns, float64 numpy arrays over the M points: ``mean``
    (d, M), ``cov`` (d, d, M), ``std`` the square root of its diagonal, ``cdf`` (d, M) the weighted
    posterior CDF ``Σ w·[draw[k] < x[k]] / Σ w`` at the points when they were given (else
    ``None``), ``ess`` (M,) ``= (Σ w)²/Σ w²``, and ``n_draws``."""

    def __init__(self, mean, cov, cdf, ess, n_draws: int):
        self.mean, self.cov, self.cdf, self.ess, self.n_draws = mean, cov, cdf, ess, int(n_draws)

    @property
    def std(self) -> np.ndarray:
        d = self.mean.shape[0]
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.cov[np.arange(d), np.arange(d)])

    def zscore(self, x_true) -> np.ndarray:
        """``(mean − x_true) / std`` per dimension and point."""
        x_true = np.asarray(x_true, dtype=np.float64)
        if x_true.shape != self.mean.shape:
            raise _lib.DimensionMismatch(f"x_true must have size {self.mean.shape}, got {x_true.shape}")
        return (self.mean - x_true) / self.std

    def __repr__(self):
        return f"WeightedPointStats(d={self.mean.shape[0]}, points={self.mean.shape[1]}, n_draws={self.n_draws})"


def weighted_moments_from_sums(block, d: int, ddof: int = 1):
    """``(mean (d, M), cov (d, d, M), ess (M,))`` in float64 from the M blocks of
    ``df_draw_weighted_stats``' ``sums_out`` — ``W1 = Σ w``, ``W2 = Σ w²``, the shift ``c``,
    ``S1w = Σ w (v − c)`` and the lower triangle of ``S2w = Σ w (v − c)(v − c)ᵀ``:
    ``mean = c + δ`` with ``δ = S1w/W1`` and
    ``cov = (S2w/W1 − δδᵀ) / (1 − W2/W1²)``, the reliability-weights correction, evaluated as
    ``(S2w − S1w S1wᵀ/W1) / (W1 − W2/W1)`` — with unit weights the very operations of
    :func:`moments_from_sums`; ``ddof=0`` divides by ``W1`` instead.  ``ess = W1²/W2``."""
    S = 2 + 2 * d + d * (d + 1) // 2
    blk = np.asarray(block, dtype=np.float64).reshape(-1, S)
    w1, w2 = blk[:, 0], blk[:, 1]
    c, s1 = blk[:, 2:2 + d], blk[:, 2 + d:2 + 2 * d]
    a, b = np.tril_indices(d)                 # row-major lower triangle: index a(a+1)/2 + b
    s2 = np.empty((blk.shape[0], d, d))
    s2[:, a, b] = blk[:, 2 + 2 * d:]
    s2[:, b, a] = blk[:, 2 + 2 * d:]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = (w1 - w2 / w1) if ddof else w1
        cov = (s2 - s1[:, :, None] * s1[:, None, :] / w1[:, None, None]) / den[:, None, None]
        mean = c + s1 / w1[:, None]
        ess = w1 * w1 / w2
    return mean.T, np.moveaxis(cov, 0, -1), ess


def weighted_stats(draws, weights, x=None, ddof: int = 1, device=None) -> WeightedPointStats:
    """The weighted mean, covariance and CDF value per point of draws under importance weights,
    reduced on the device (``df_draw_weighted_stats``) → :class:`WeightedPointStats`.  ``draws`` is
    a numpy ``(M, N, d)`` Float32 array or a device tensor of that shape in C order (the layout of
    :func:`posterior_draws`); ``N`` a multiple of 4, ``d <= 64``.  ``weights`` is an
    :class:`ImportanceWeights` or an ``(M, N)`` Float32 array or tensor of finite weights ``>= 0``
    (not checked).  ``x`` (d, M), when given, are the points of the weighted SBC statistic ``cdf``
    (a Float32 ``<``: a tie or a NaN counts nothing).  ``ddof`` as for
    :func:`weighted_moments_from_sums`.  With unit weights the sums are those of
    :func:`posterior_stats` bit for bit."""
    import torch

    from .hip import run_draw_weighted_stats

    is_t = isinstance(draws, torch.Tensor)
    if not is_t:
        draws = np.asarray(draws)
    if draws.dtype != (torch.float32 if is_t else np.float32):
        raise _lib.ArgumentError(f"draws must be Float32 (got {draws.dtype})")
    if len(draws.shape) != 3:
        raise _lib.DimensionMismatch(f"draws must have size (M, N, d), got {tuple(draws.shape)}")
    M, N, d = (int(v) for v in draws.shape)
    if not 1 <= d <= 64:
        raise _lib.ArgumentError("d must be in 1 .. 64")
    if isinstance(weights, ImportanceWeights):
        wsrc = weights._device_w if weights._device_w is not None else weights.w
    else:
        wsrc = weights
    _check_mn(wsrc, "weights", (M, N))
    if x is not None:
        if not isinstance(x, torch.Tensor):
            x = np.asarray(x)
        if len(x.shape) < 1 or int(x.shape[0]) != d or int(np.prod(x.shape[1:])) != M:
            raise _lib.DimensionMismatch(f"x must have size ({d}, {M}), got {tuple(x.shape)}")
    dev = torch.device(device) if device is not None else _default_device(draws, wsrc)
    xs = _device_rows(draws, dev)
    wb = _device_rows(wsrc, dev)
    xb = as_julia_device(x, d, dev, "x")[0] if x is not None else None
    S = 2 + 2 * d + d * (d + 1) // 2
    sums = torch.empty((M, S), dtype=torch.float64, device=dev)
    wrank = torch.empty((M, d), dtype=torch.float64, device=dev) if x is not None else None
    if M > 0:
        run_draw_weighted_stats(xs, wb, xb, d, M, N, wrank, sums)
    torch.cuda.synchronize(dev)
    blk = sums.cpu().numpy()
    mean, cov, ess = weighted_moments_from_sums(blk, d, ddof)
    cdf = None
    if x is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            cdf = (wrank.cpu().numpy() / blk[:, :1]).T
    return WeightedPointStats(mean, cov, cdf, ess, N)


def importance_posterior_stats(flow: Flow, theta, log_target, n_draws: int = 1024, x=None, dims=None, rng=None,
                               seed: Optional[int] = None, offset: int = 0, ddof: int = 1):
    """Importance-corrected posterior summaries of a conditional flow →
    ``(WeightedPointStats, ImportanceWeights)``: :func:`posterior_draws` on the device, the
    caller's ``log_target(draws, theta)`` — the unnormalised log-posterior at the draws, a device
    tensor ``(M, N, d)`` in and a Float32 device tensor ``(M, N)`` out — then
    :func:`importance_weights` against the draws' ``log q`` and :func:`weighted_stats` under those
    weights, with the weighted CDF at the points ``x`` (d, dims...) when given.  Between the draw
    and the per-point blocks nothing leaves the device; the result is bitwise the composition of
    the three calls.  ``theta``, ``dims``, ``n_draws`` and the seed arguments as for
    :func:`posterior_stats`."""
    dims = _check_point_draws(flow, x, theta, n_draws, 0, dims)
    draws, lq = posterior_draws(flow, theta, n_draws=n_draws, dims=dims, rng=rng, seed=seed, offset=offset,
                                as_tensor=True)
    iw = importance_weights(log_target(draws, theta), lq)
    return weighted_stats(draws, iw, x, ddof=ddof), iw


# ---------------------------------------------------------------------------
# importance resampling: exact picks and gathered draws (df_resample.hip)
# ---------------------------------------------------------------------------

RESAMPLE_METHODS = {"systematic": 0, "stratified": 1, "multinomial": 2}
RESAMPLE_LDS_DRAWS = 4096          # DF_RESAMPLE_LDS_DRAWS: above it the call needs a workspace


def _check_resample(weights, n_out, method):
    """The host checks of a resampling call, no library call → ``(weights array, M, N, K, method
    code)``."""
    if not isinstance(method, str) or method not in RESAMPLE_METHODS:
        raise _lib.ArgumentError(f"unknown resampling method {method!r}: one of {', '.join(RESAMPLE_METHODS)}")
    if isinstance(weights, ImportanceWeights):
        wsrc = weights._device_w if weights._device_w is not None else weights.w
    else:
        wsrc = weights
    M, N = _check_mn(wsrc, "weights")
    K = _check_n_out(n_out, N)
    return wsrc, M, N, K, RESAMPLE_METHODS[method]


def _check_n_out(n_out, N: int) -> int:
    K = N if n_out is None else int(n_out)
    if K <= 0 or K % 4 != 0:
        raise _lib.ArgumentError("n_out must be a positive multiple of 4")
    if K > MAX_CHUNK:
        raise _lib.UnsupportedError("a point has at most 2^24 picks (n_out)")
    return K


def _run_resample(xs, wsrc, d, M, N, K, code, seed, offset, want_draws, want_idx, dev):
    """One ``df_draw_resample`` call on checked arguments → device tensors ``(draws (M, K, d) or
    None, indices (M, K) or None)``; nothing synchronises."""
    import torch

    from .hip import run_draw_resample

    wb = _device_rows(wsrc, dev)
    out = torch.empty((M, K, d), dtype=torch.float32, device=dev) if want_draws else None
    idx = torch.empty((M, K), dtype=torch.int32, device=dev) if want_idx else None
    ws = torch.empty((M, N), dtype=torch.int64, device=dev) if N > RESAMPLE_LDS_DRAWS else None
    if M > 0:
        run_draw_resample(xs, wb, d, M, N, K, code, seed, int(offset), out, idx, ws)
    return out, idx


def resample_indices(weights, n_out: Optional[int] = None, method: str = "systematic", rng=None,
                     seed: Optional[int] = None, offset: int = 0, device=None):
    """Per point ``n_out`` picks among its N weighted draws, on the device (``df_draw_resample``
    without the gather) → ``(M, n_out)`` int32 indices within the point, numpy for numpy weights and
    a device tensor otherwise.  ``weights`` is an :class:`ImportanceWeights` or an ``(M, N)`` Float32
    array or tensor; ``n_out`` (default N) a multiple of 4; ``method`` one of ``"systematic"``,
    ``"stratified"`` (both non-decreasing in k) and ``"multinomial"`` (stream order).  The picks are
    exact integer arithmetic on the weights quantised to 32 bits below the point's largest (the
    header states the contract): bitwise reproducible at a ``(seed, offset)``; a weight that is
    NaN, ±inf, negative or 0 is never picked, and a point without any other gives −1 throughout.
    Method, dtype, shape and ``n_out`` are checked before the library is touched."""
    import torch

    wsrc, M, N, K, code = _check_resample(weights, n_out, method)
    seed = _draw_seed(rng, seed)
    was_np = not isinstance(weights.w if isinstance(weights, ImportanceWeights) else weights, torch.Tensor)
    dev = torch.device(device) if device is not None else _default_device(wsrc)
    _, idx = _run_resample(None, wsrc, 0, M, N, K, code, seed, offset, False, True, dev)
    return idx.cpu().numpy() if was_np else idx


def resample(draws, weights, n_out: Optional[int] = None, method: str = "systematic", rng=None,
             seed: Optional[int] = None, offset: int = 0, return_indices: bool = False, device=None):
    """Weighted draws resampled to equally weighted ones, on the device (``df_draw_resample``) →
    ``(M, n_out, d)`` Float32: row k of point i is the draw :func:`resample_indices` picks, copied bit
    for bit (all-NaN where the pick is −1).  ``draws`` is a numpy ``(M, N, d)`` Float32 array or a
    device tensor of that shape in C order, ``d <= 64``; the result is numpy for numpy draws and
    stays on the device for a tensor — the layout :func:`order_statistics`, :func:`draw_histograms`
    and :func:`weighted_stats` (at unit weights) take.  The other arguments as for
    :func:`resample_indices`; with ``return_indices=True`` the value is ``(draws, indices)``."""
    import torch

    is_t = isinstance(draws, torch.Tensor)
    if not is_t:
        draws = np.asarray(draws)
    if draws.dtype != (torch.float32 if is_t else np.float32):
        raise _lib.ArgumentError(f"draws must be Float32 (got {draws.dtype})")
    if len(draws.shape) != 3:
        raise _lib.DimensionMismatch(f"draws must have size (M, N, d), got {tuple(draws.shape)}")
    d = int(draws.shape[2])
    if not 1 <= d <= 64:
        raise _lib.ArgumentError("d must be in 1 .. 64")
    wsrc, M, N, K, code = _check_resample(weights, n_out, method)
    if (M, N) != tuple(int(v) for v in draws.shape[:2]):
        raise _lib.DimensionMismatch(f"weights must have size {tuple(draws.shape[:2])}, got {(M, N)}")
    seed = _draw_seed(rng, seed)
    dev = torch.device(device) if device is not None else _default_device(draws, wsrc)
    out, idx = _run_resample(_device_rows(draws, dev), wsrc, d, M, N, K, code, seed, offset, True,
                             bool(return_indices), dev)
    if not is_t:
        out = out.cpu().numpy()
        idx = idx.cpu().numpy() if return_indices else None
    return (out, idx) if return_indices else out


def importance_resample(flow: Flow, theta, log_target, n_draws: int = 1024, n_out: Optional[int] = None,
                        method: str = "systematic", dims=None, rng=None, seed: Optional[int] = None, offset: int = 0,
                        as_tensor: bool = False):
    """Equally weighted draws of the importance-corrected posterior of a conditional flow →
    ``(draws (M, n_out, d), ImportanceWeights)``: :func:`posterior_draws` on the device, the caller's
    ``log_target(draws, theta)`` as for :func:`importance_posterior_stats`, :func:`importance_weights`
    against the draws' ``log q`` and :func:`resample` under those weights, with nothing leaving the
    device in between; the result is bitwise the composition of the four calls at the same
    ``(seed, offset)`` (the resampler's Philox stream is disjoint from the draw's).  ``n_out``
    defaults to ``n_draws``; numpy unless ``as_tensor``.  ``theta``, ``dims``, ``n_draws`` and the
    seed arguments as for :func:`posterior_stats`; ``method`` and ``n_out`` as for
    :func:`resample_indices`, checked before the library is touched."""
    if not isinstance(method, str) or method not in RESAMPLE_METHODS:
        raise _lib.ArgumentError(f"unknown resampling method {method!r}: one of {', '.join(RESAMPLE_METHODS)}")
    dims = _check_point_draws(flow, None, theta, n_draws, 0, dims)
    _check_n_out(n_out, int(n_draws))
    seed = _draw_seed(rng, seed)
    draws, lq = posterior_draws(flow, theta, n_draws=n_draws, dims=dims, seed=seed, offset=offset, as_tensor=True)
    iw = importance_weights(log_target(draws, theta), lq)
    out = resample(draws, iw, n_out=n_out, method=method, seed=seed, offset=offset)
    return (out if as_tensor else out.cpu().numpy()), iw


# ---------------------------------------------------------------------------
# weighted quantiles and histograms: fixed-point weights, exact (df_wquant.hip, df_whist.hip)
# ---------------------------------------------------------------------------

WQUANT_MAX_PROBS = 32              # DF_WQUANT_MAX_PROBS
WHIST_MAX_TABLE_BINS = 8192        # DF_WHIST_MAX_TABLE_BINS


def quantile_numerators(probs):
    """The numerators of the weighted-quantile call: ``num = int(rint(float64(p)·2^32))`` over the
    fixed denominator 2^32, a list of Python ints in ``[0, 2^32]``.  Probabilities outside [0, 1],
    NaN, none and more than 32 are refused.  No library call."""
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64)).reshape(-1)
    if p.size == 0:
        raise _lib.ArgumentError("no probabilities")
    if not np.all((p >= 0.0) & (p <= 1.0)):            # a NaN fails both comparisons
        raise _lib.ArgumentError("probabilities must lie in [0, 1]")
    if p.size > WQUANT_MAX_PROBS:
        raise _lib.ArgumentError(f"{p.size} probabilities, at most {WQUANT_MAX_PROBS} in one call")
    return [int(v) for v in np.rint(p * 4294967296.0)]


def _check_weighted_draws(draws, weights):
    """The host checks the weighted per-point calls share, no library call → ``(weights array, M, N,
    d, draws are a tensor)``."""
    import torch

    is_t = isinstance(draws, torch.Tensor)
    if not is_t:
        draws = np.asarray(draws)
    if draws.dtype != (torch.float32 if is_t else np.float32):
        raise _lib.ArgumentError(f"draws must be Float32 (got {draws.dtype})")
    if len(draws.shape) != 3:
        raise _lib.DimensionMismatch(f"draws must have size (M, N, d), got {tuple(draws.shape)}")
    M, N, d = (int(v) for v in draws.shape)
    if not 1 <= d <= 64:
        raise _lib.ArgumentError("d must be in 1 .. 64")
    wsrc = _weights_source(weights)
    _check_mn(wsrc, "weights", (M, N))
    return wsrc, M, N, d, is_t


def _weights_source(weights):
    if isinstance(weights, ImportanceWeights):
        return weights._device_w if weights._device_w is not None else weights.w
    return weights


def weight_scale(weights, device=None):
    """The fixed-point scale of every point's weights, on the device (``df_draw_weight_scale``) →
    ``(e, T)``, int64 numpy vectors of length M: with ``wmax = f·2^e``, ``f`` in [0.5, 1), the
    largest finite weight ``> 0`` of the point, ``q_j = rint(w_j·2^(32 − e))`` (half to even; 0 for
    NaN, ±inf, negative and ±0 weights) and ``T = Σ q_j``.  A point without a weight that takes
    part is empty: ``(0, 0)``.  ``weights`` is an :class:`ImportanceWeights` or an ``(M, N)`` Float32
    array or tensor, as for :func:`resample`."""
    import torch

    from .hip import run_draw_weight_scale

    wsrc = _weights_source(weights)
    M, N = _check_mn(wsrc, "weights")
    dev = torch.device(device) if device is not None else _default_device(wsrc)
    wb = _device_rows(wsrc, dev)
    scale = torch.empty((M, 2), dtype=torch.int64, device=dev)
    if M > 0:
        run_draw_weight_scale(wb, M, N, scale)
    torch.cuda.synchronize(dev)
    s = scale.cpu().numpy()
    return s[:, 0].copy(), s[:, 1].copy()


def _run_weighted_quantiles(draws, wsrc, M, N, d, nums, dev):
    """One ``df_draw_weighted_quantiles`` call on checked arguments → device tensors ``(quantiles
    (M, d, P) float32, scale (M, 2) int64)``; nothing synchronises."""
    import torch

    from .hip import run_draw_weighted_quantiles

    xs = _device_rows(draws, dev)
    wb = _device_rows(wsrc, dev)
    out = torch.empty((M, d, len(nums)), dtype=torch.float32, device=dev)
    scale = torch.empty((M, 2), dtype=torch.int64, device=dev)
    if M > 0:
        run_draw_weighted_quantiles(xs, wb, d, M, N, nums, out, scale)
    return out, scale


def weighted_quantiles(draws, weights, probs=(0.16, 0.5, 0.84), device=None):
    """The weighted quantiles ``probs`` of every dimension of every point's draws under importance
    weights, selected on the device (``df_draw_weighted_quantiles``) → float32 ``(M, d, P)``, a numpy
    array for numpy draws and a device tensor otherwise.  ``draws`` is a numpy ``(M, N, d)`` Float32
    array or a device tensor of that shape in C order (the layout of :func:`posterior_draws`);
    ``N`` a multiple of 4, ``d <= 64``.  ``weights`` is an :class:`ImportanceWeights` or an ``(M, N)``
    Float32 array or tensor.  The rule is the inverted CDF on the quantised weights ``q_j`` of
    :func:`weight_scale` — numpy's ``method="inverted_cdf"`` with ``weights=q``: with
    ``τ = max(1, ceil(num·T / 2^32))`` (``num`` of :func:`quantile_numerators`) the draw with the
    smallest totalOrder key ``k`` such that ``Σ {q_j : key_j <= k} >= τ``, bit for bit — integer
    arithmetic, no interpolation, no resampling noise.  ``p = 0`` gives the smallest and ``p = 1``
    the largest draw with a weight that takes part; NaN draws sort to the ends; an empty point
    gives NaN.  Dtype, shape and probabilities are checked before the library is touched."""
    import torch

    wsrc, M, N, d, is_t = _check_weighted_draws(draws, weights)
    nums = quantile_numerators(probs)
    dev = torch.device(device) if device is not None else _default_device(draws, wsrc)
    out, _ = _run_weighted_quantiles(draws, wsrc, M, N, d, nums, dev)
    if is_t:
        return out
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def _interval_probs(level):
    level = float(level)
    if not 0.0 < level < 1.0:                                 # a NaN fails both comparisons
        raise _lib.ArgumentError("level must lie in (0, 1)")
    return ((1.0 - level) / 2, 0.5, (1.0 + level) / 2)


def weighted_credible_intervals(draws, weights, level: float = 0.68, device=None):
    """The equal-tailed weighted credible interval of every point and dimension →
    ``(lower, median, upper)``, each float32 ``(M, d)``: :func:`weighted_quantiles` at
    ``probs = ((1 − level)/2, 0.5, (1 + level)/2)``; ``0 < level < 1``."""
    q = weighted_quantiles(draws, weights, _interval_probs(level), device=device)
    return q[:, :, 0], q[:, :, 1], q[:, :, 2]


class WeightedPointHistograms:
    """What :func:`weighted_histograms` returns: ``tables``, the dict
    ``{(a,): (M, L_a), (a, b): (M, L_a, L_b)}`` of uint64 numpy arrays — per bin the sum of the
    quantised weights of its draws — over the M points, ``edges`` (d Float32 vectors, ``None`` for a
    dimension without bins), the int64 vectors ``e`` and ``T`` of :func:`weight_scale` that give the
    sums their unit, ``n_draws`` and ``dims``."""

    def __init__(self, tables, edges, e, T, n_draws: int, dims=()):
        self.tables, self.edges, self.n_draws, self.dims = tables, edges, int(n_draws), tuple(dims)
        self.e, self.T = np.asarray(e, np.int64), np.asarray(T, np.int64)

    _key = staticmethod(PointHistograms._key)

    def _per_point(self, v, K):
        return v.reshape((-1,) + (1,) * len(K))

    def sums(self, K) -> np.ndarray:
        """The uint64 bins of the table."""
        return self.tables[self._key(K)]

    def mass(self, K) -> np.ndarray:
        """``sums · 2^(e − 32)`` in float64: the bins in the units of the caller's weights."""
        K = self._key(K)
        return np.ldexp(self.tables[K].astype(np.float64), self._per_point((self.e - 32).astype(np.int32), K))

    def inside(self, K) -> np.ndarray:
        """The quantised weight inside the table's range per point, uint64 (M,): its sum."""
        c = self.tables[self._key(K)]
        return c.reshape(c.shape[0], -1).sum(axis=1, dtype=np.uint64)

    def density(self, K) -> np.ndarray:
        """``sums / (T · bin width)`` (1-D) or ``/ (T · bin area)`` (2-D) in float64: it integrates
        to the inside fraction ``inside(K) / T``.  A bin with an infinite edge has density 0; an
        empty point gives NaN."""
        K = self._key(K)
        w = np.diff(self.edges[K[0]].astype(np.float64))
        if len(K) == 2:
            w = w[:, None] * np.diff(self.edges[K[1]].astype(np.float64))[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.tables[K].astype(np.float64) / (self._per_point(self.T.astype(np.float64), K) * w)

    def pooled(self, K) -> np.ndarray:
        """``Σ_i sums_i / T_i`` in float64 over the points that are not empty: every point enters
        with total weight 1."""
        K = self._key(K)
        ok = self.T > 0
        return (self.tables[K][ok].astype(np.float64) / self._per_point(self.T[ok].astype(np.float64), K)).sum(axis=0)

    def __repr__(self):
        return f"WeightedPointHistograms(tables={len(self.tables)}, dims={self.dims}, n_draws={self.n_draws})"


def weighted_histograms(draws, weights, edges, keep=None, device=None) -> WeightedPointHistograms:
    """The 1-D and 2-D marginal histograms of every point's draws under importance weights, summed
    on the device (``df_draw_weighted_histograms``) → :class:`WeightedPointHistograms`.  ``draws``,
    ``edges`` and ``keep`` as for :func:`draw_histograms` (the same bin rule and tables; a table
    holds at most 8192 bins), ``weights`` as for :func:`weighted_quantiles`.  A bin holds ``Σ q_j``
    of the draws :func:`draw_histograms` would have counted there, with the quantised weights
    ``q_j`` of :func:`weight_scale`, as uint64: integer sums, the same bytes whatever the kernel
    mapping.  With unit weights every table is the count table shifted left by 31."""
    import torch

    from .hip import run_draw_weighted_histograms

    wsrc, M, N, d, is_t = _check_weighted_draws(draws, weights)
    ev, bins = histogram_edges(edges, d)
    reqs = _histogram_requests(keep, bins)
    for K in reqs:
        size = int(np.prod([bins[k] for k in K]))
        if size > WHIST_MAX_TABLE_BINS:
            raise _lib.UnsupportedError(f"keep {K}: a table of {size} bins is above {WHIST_MAX_TABLE_BINS}")
    T = sum(int(np.prod([bins[k] for k in K])) for K in reqs)
    dev = torch.device(device) if device is not None else _default_device(draws, wsrc)
    xs = _device_rows(draws, dev)
    wb = _device_rows(wsrc, dev)
    eb = torch.from_numpy(np.concatenate([v for v in ev if v is not None])).to(dev)
    out = torch.empty((M, T), dtype=torch.int64, device=dev)
    scale = torch.empty((M, 2), dtype=torch.int64, device=dev)
    if M > 0:
        run_draw_weighted_histograms(xs, wb, d, M, N, eb, bins, reqs, out, scale)
    torch.cuda.synchronize(dev)
    s = scale.cpu().numpy()
    tables = _histogram_tables(out.cpu().numpy().view(np.uint64), M, reqs, bins)
    return WeightedPointHistograms(tables, ev, s[:, 0].copy(), s[:, 1].copy(), N)


def _importance_draws(flow: Flow, theta, log_target, n_draws, dims, rng, seed, offset):
    """:func:`posterior_draws`, the caller's closure and :func:`importance_weights`, all on the
    device → ``(draws tensor, ImportanceWeights, dims)``."""
    dims = _check_point_draws(flow, None, theta, n_draws, 0, dims)
    draws, lq = posterior_draws(flow, theta, n_draws=n_draws, dims=dims, rng=rng, seed=seed, offset=offset,
                                as_tensor=True)
    return draws, importance_weights(log_target(draws, theta), lq), dims


def importance_posterior_quantiles(flow: Flow, theta, log_target, probs=(0.16, 0.5, 0.84), n_draws: int = 1024,
                                   dims=None, rng=None, seed: Optional[int] = None, offset: int = 0):
    """Importance-corrected posterior quantiles of a conditional flow →
    ``(quantiles (M, d, P) float32 numpy, ImportanceWeights)``: :func:`posterior_draws` on the
    device, the caller's ``log_target(draws, theta)`` as for :func:`importance_posterior_stats`,
    :func:`importance_weights` against the draws' ``log q`` and :func:`weighted_quantiles` under
    those weights, with nothing leaving the device in between; the result is bitwise the
    composition of the three calls.  The probabilities are checked before the library is touched;
    ``theta``, ``dims``, ``n_draws`` and the seed arguments as for :func:`posterior_stats`."""
    quantile_numerators(probs)
    draws, iw, _ = _importance_draws(flow, theta, log_target, n_draws, dims, rng, seed, offset)
    return weighted_quantiles(draws, iw, probs).cpu().numpy(), iw


def importance_credible_intervals(flow: Flow, theta, log_target, level: float = 0.68, n_draws: int = 1024, dims=None,
                                  rng=None, seed: Optional[int] = None, offset: int = 0):
    """``((lower, median, upper), ImportanceWeights)``, each bound float32 ``(M, d)``:
    :func:`importance_posterior_quantiles` at ``probs = ((1 − level)/2, 0.5, (1 + level)/2)``."""
    q, iw = importance_posterior_quantiles(flow, theta, log_target, _interval_probs(level), n_draws, dims, rng, seed,
                                           offset)
    return (q[:, :, 0], q[:, :, 1], q[:, :, 2]), iw


def importance_posterior_histograms(flow: Flow, theta, log_target, edges=None, keep=None, n_draws: int = 1024,
                                    dims=None, rng=None, seed: Optional[int] = None, offset: int = 0):
    """The importance-corrected corner plot of a conditional flow →
    ``(WeightedPointHistograms, ImportanceWeights)``: the chain of
    :func:`importance_posterior_quantiles` with :func:`weighted_histograms` at its end; ``edges``
    and ``keep`` as there, checked before the library is touched."""
    if edges is None:
        raise _lib.ArgumentError("importance_posterior_histograms needs edges: one entry per dimension")
    _histogram_requests(keep, histogram_edges(edges, flow.d)[1])
    draws, iw, dims = _importance_draws(flow, theta, log_target, n_draws, dims, rng, seed, offset)
    res = weighted_histograms(draws, iw, edges, keep)
    res.dims = tuple(dims)
    return res, iw


def pdf(flow: Flow, x, theta=None):
    """``pdf = exp.(logpdf)`` — src/Flows.jl:345-349."""
    lp = logpdf(flow, x, theta)
    return np.exp(lp) if isinstance(lp, np.ndarray) else lp.exp()


def nll_partial_sum(flow: Flow, x, theta=None, out=None):
    """Σ_j logpdf(x_j) in fp64 on device (deterministic), plus the sample count —
    the per-rank partial of ``loss`` (src/Flows.jl:352-359)."""
    th = flow._theta(theta, x, device=True)
    return flow.hip().logpdf_sum(x, th, out=out)


def training_loss(flow: Flow):
    return flow.train_loss


def validation_loss(flow: Flow):
    return flow.valid_loss
