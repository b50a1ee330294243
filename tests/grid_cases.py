"""Grids of the grid-logpdf tests (tests/test_grid_host.py on the CPU, tests/test_gpu_grid.py
on the GPU): the chains of tests/edge_cases.py with axis vectors taken from their own
inputs, a numpy enumerator of the grid's points, and the fp64 oracle of each grid computed
once.  Plain numpy, read-only.

An axis of length L > 1 holds the quantiles 0.2 … 0.8 of that dimension of the case's
`x_in` (`th_raw` for a θ axis), an axis of length 1 its median: the grid lies where the
flow puts its data, so the 1e-5 criterion is one the oracle's own fp32 arithmetic keeps
(test_grid_host.py::test_grid_fp32_oracle)."""
import numpy as np

import edge_cases as E
from oracle import flow_oracle as O

LENS5 = (3, 1, 5, 2, 7)                                   # coprime, with a length-1 axis: 210 points
LENS_X = {5: LENS5, 6: LENS5 + (2,), 7: LENS5 + (2, 1),   # 420 points
          12: (3, 1, 2, 1, 2, 1, 3, 1, 2, 1, 2, 1)}       # 144 points
LENS_MANY = (7, 5, 3, 4, 3)                               # 1260 points: more than two workgroups
README16 = "readme16"                                     # the fast16 chain created with no environment

# test 1 of test_gpu_grid.py: case -> x lengths (θ: one value per condition)
BITWISE_CASES = ("generic_custom", "uniform_tanh32", "slowcopy_d12", "fast16", README16, "split64", "split32",
                 "wide_split", "norm_only_d5")
# test 4: case -> θ lengths
THETA_AXES = {"split32": (1, 3), "wide_split": (2, 1)}
# test 3: five axes of 128 values, P = 2³⁵, and a window past point 2³³
BIG_LEN, BIG_FIRST, BIG_COUNT = 128, 2**33 + 5, 300
# strides 1, 2¹⁶, 2³², 3·2³², 6·2³² (past 32 bits) and a window in which all three of the
# slow axes step at once
HUGE_LENS, HUGE_FIRST = (65536, 65536, 3, 2, 2), 6 * 2**32 - 100


def edge_name(name):
    return "fast16" if name == README16 else name


def case_dims(name):
    entry = E.CASES.get(edge_name(name)) or E.NORM_ONLY[edge_name(name)]
    return entry[1], entry[2]


def axis(values, L):
    """L values of one dimension: its quantiles 0.2 … 0.8, the median for L = 1."""
    v = np.asarray(values, np.float64)
    q = np.median(v) if L == 1 else np.quantile(v, np.linspace(0.2, 0.8, L))
    return np.atleast_1d(q).astype(np.float32)


def case_axes(name, lens_x, lens_th=None):
    """(x axes, θ axes) of a case; lens_th None: one value per condition."""
    D = E.case_data(edge_name(name))
    assert len(lens_x) == D["d"]
    lens_th = (1,) * D["n"] if lens_th is None else tuple(lens_th)
    assert len(lens_th) == D["n"]
    xa = [axis(D["x_in"][k], L) for k, L in enumerate(lens_x)]
    ta = [axis(D["th_raw"][k], L) for k, L in enumerate(lens_th)]
    return xa, ta


def grid_points(axes, first=0, count=None):
    """Points [first, first + count) of the outer product of `axes` as a (len(axes), count)
    float32 array, the first axis varying fastest (Iterators.product order)."""
    lens = [int(len(a)) for a in axes]
    P = int(np.prod(lens, dtype=object)) if lens else 1
    count = P - first if count is None else count
    assert 0 <= first and first + count <= P and P < 2**62
    p = first + np.arange(count, dtype=np.int64)
    out = np.empty((len(axes), count), np.float32)
    stride = 1
    for k, a in enumerate(axes):
        out[k] = np.asarray(a, np.float32)[(p // stride) % lens[k]]
        stride *= lens[k]
    return out


_CACHE = {}


def grid_data(name, lens_x, lens_th=None, first=0, count=None):
    """Axes, materialised points and the fp64 oracle of one grid (window), computed once."""
    key = (name, tuple(lens_x), None if lens_th is None else tuple(lens_th), first, count)
    if key in _CACHE:
        return _CACHE[key]
    D = E.case_data(edge_name(name))
    d, n = D["d"], D["n"]
    xa, ta = case_axes(name, lens_x, lens_th)
    pts = grid_points(xa + ta, first, count)
    x, th_raw = pts[:d], pts[d:]
    th = O.normalize_input(th_raw, D["tmin"], D["tmax"]) if n else np.zeros((0, pts.shape[1]), np.float32)
    lp = O.flow_logpdf(D["spec"], x, th, np.float64)
    out = dict(d=d, n=n, x_axes=xa, th_axes=ta, lens=tuple(len(a) for a in xa + ta), x=x, th_raw=th_raw, th=th,
               lp=lp, spec=D["spec"], tmin=D["tmin"], tmax=D["tmax"])
    for v in list(out.values()) + xa + ta:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = out
    return out


def all_grids():
    """Every grid the GPU tests evaluate: (id, grid_data arguments)."""
    out = []
    for name in BITWISE_CASES:
        out.append((name, (name, LENS_X[case_dims(name)[0]])))
    out.append(("split64-many", ("split64", LENS_MANY)))
    out.append(("split64-2^33", ("split64", (BIG_LEN,) * 5, None, BIG_FIRST, BIG_COUNT)))
    out.append(("split64-strides-2^32", ("split64", HUGE_LENS, None, HUGE_FIRST, BIG_COUNT)))
    for name, lt in THETA_AXES.items():
        out.append((f"{name}-theta", (name, LENS_X[case_dims(name)[0]], lt)))
    return out
