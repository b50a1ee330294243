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

__all__ = ["Flow", "MvNormal", "predict", "sample", "logpdf", "logpdf_grid", "logpdf_grad", "pdf",
           "training_loss", "validation_loss", "nll_partial_sum"]

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


def _grid_eval(flow: Flow, x_axes, theta_axes, first, count, chunk):
    """Shared by logpdf_grid and the tuple-x logpdf → (flat device values, lens, numpy out?,
    whole grid?)."""
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
    P = 1
    for L in lens:
        P *= L
    whole = first == 0 and count is None
    first = int(first)
    count = P - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > P:
        raise _lib.DimensionMismatch(f"window [{first}, {first + count}) outside the grid of {P} points")
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
        # A new trainer starts from the parameters the chain was planned with: hand the chain
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
