"""The planner's output, byte for byte: tests/plan_fingerprint.cpp links df_plan.cpp, plans
one serialised chain descriptor and prints every scalar of df::Plan and a hash of every
vector of it (or the status and message of a refused descriptor).  This test plans the
matrix below and compares every line with tests/golden/plan_fingerprint.json.

The expectations were recorded from the df_plan.cpp of commit 98194e2, BEFORE the planner's
internals were rewritten (one stage writer, one parameter sink per blob, two fragment
walkers, build_plan in passes), by the same program:

    python tests/test_plan_fingerprint.py --record <path to that df_plan.cpp>

Regenerate only when a change is MEANT to alter a blob layout, a descriptor or an error,
from the planner BEFORE that change plus a reasoned diff, never from the code under test.

The program is compiled with -fsanitize=address,undefined and run as a child process (no
GPU, no code loaded into Python); DF_* variables are cleared but for the case's own."""
import copy
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import densityflows_amd as dfa  # noqa: E402
from densityflows_amd import _lib, hip  # noqa: E402
from densityflows_amd.layers import NormalizationLayer, RNVPCouplingLayer  # noqa: E402
from helpers import _single_dense_spec, spec_to_element  # noqa: E402
from oracle import flow_oracle as O  # noqa: E402

import edge_cases as E  # noqa: E402
import make_head_pin as HP  # noqa: E402

CSRC = os.path.join(ROOT, "densityflows.jl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "plan_fingerprint.json")


# ---------------------------------------------------------------------------
# descriptors: plain dicts (so that a refused one can be written too) and their file form
# ---------------------------------------------------------------------------

def describe(elements, n_hint=None):
    """The descriptor hip._Desc builds for a chain, as plain data."""
    flat = hip.flatten_elements(elements)
    d, n = hip.chain_dims(flat, n_hint)

    def net(chain):
        return [{"in": D.in_dim, "out": D.out_dim, "act": _lib.ACTIVATIONS[D.act],
                 "W": np.asfortranarray(D.W, dtype=np.float32),
                 "b": None if D.b is None else np.ascontiguousarray(D.b, dtype=np.float32)} for D in chain]

    layers = []
    for e_idx, l in flat:
        if isinstance(l, NormalizationLayer):
            layers.append({"kind": _lib.DF_LAYER_NORM, "element": e_idx, "alpha": l.alpha, "beta": l.beta,
                           "x_min": np.asarray(l.x_min, np.float32), "x_max": np.asarray(l.x_max, np.float32)})
            continue
        rnvp = isinstance(l, RNVPCouplingLayer)
        layers.append({"kind": _lib.DF_LAYER_RNVP if rnvp else _lib.DF_LAYER_NICE, "element": e_idx,
                       "axis_af": list(l.axes.axis_af), "axis_nn": list(l.axes.axis_nn),
                       "s_net": net(l.s_net) if rnvp else [], "t_net": net(l.t_net)})
    return {"abi": _lib.ABI_VERSION, "d": d, "n": n, "layers": layers}


def serialise(desc, path):
    """The word stream tests/plan_fingerprint.cpp reads (floats as their bits)."""
    parts = []

    def ints(*v):
        parts.append(np.asarray(v, dtype="<i4").ravel())

    def floats(a):
        parts.append(np.ascontiguousarray(a, dtype="<f4").ravel().view("<i4"))

    ints(desc["abi"], desc["d"], desc["n"], len(desc["layers"]))
    for L in desc["layers"]:
        ints(L["kind"], L["element"])
        if L["kind"] == _lib.DF_LAYER_NORM:
            floats([L["alpha"], L["beta"]])
            floats(L["x_min"])
            floats(L["x_max"])
            continue
        ints(len(L["axis_af"]), *L["axis_af"])
        ints(len(L["axis_nn"]), *L["axis_nn"])
        for net in (L["s_net"], L["t_net"]):
            ints(len(net))
            for D in net:
                ints(D["in"], D["out"], D["act"], 0 if D["b"] is None else 1)
                floats(np.asarray(D["W"]).ravel(order="F"))   # (out, in) column-major
                if D["b"] is not None:
                    floats(D["b"])
    np.concatenate(parts).tofile(path)


# ---------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------

def _bench_configs(seed=0):
    """Configurations 2, 1 and 4 as tests/test_host.py builds them, seed 0 (another seed: the
    same structures with other parameters, tests/test_repack_closure.py)."""
    rng = np.random.default_rng(seed)
    ch2 = dfa.FlowChain.repeat(dfa.CouplingBlock, 4, 5, hidden_dim_s=64, hidden_dim_t=64, rng=rng)
    x = np.load(os.path.join(HERE, "golden", "datatest_x.npy"))
    th = np.load(os.path.join(HERE, "golden", "datatest_theta.npy"))
    data = dfa.DataArrays(x, th, rng=rng)
    ch1 = dfa.FlowChain(*[dfa.CouplingLayer(data, m, hidden_dim_s=16, hidden_dim_t=16, rng=rng)
                          for m in ([1, 2, 3], [3, 4, 5], [5, 1, 2])],
                        dfa.NormalizationLayer.from_data(x, -1.0, 1.0))
    rng = np.random.default_rng(seed)
    ch4 = dfa.FlowChain.repeat(dfa.CouplingBlock, 8, 32, n=8, hidden_dim_s=256, hidden_dim_t=256, rng=rng)
    return {"cfg1": describe(ch1.layers), "cfg2": describe(ch2.layers), "cfg4": describe(ch4.layers)}


def _spec_chain(rng, d, n, masks, bias=True, **kw):
    layers = [O.rnvp_layer(rng, O.coupling_axes(d, m, n=n), bias_scale=0.1, out_scale=0.5, **kw) for m in masks]
    if not bias:
        for L in layers:
            for D in L["s_net"] + L["t_net"]:
                D["b"] = None
    return describe(spec_to_element({"kind": "chain", "layers": layers}).layers)


_MASKS = ([1, 2, 3], [4, 5], [5, 1, 2])


def _small(seed=7, **kw):
    return lambda: _spec_chain(np.random.default_rng(seed), 5, 1, _MASKS, **kw)


def _wide_first():
    """40 conditioner inputs at hidden 256: the first Dense takes two wide stages, and the
    split feature table is padded to 64."""
    masks = (list(range(1, 17)), list(range(17, 33)))
    return _spec_chain(np.random.default_rng(8), 32, 24, masks, hidden=256)


def _failing():
    """name: a refused descriptor (each a valid chain with one thing wrong)."""
    def base():
        return _spec_chain(np.random.default_rng(9), 5, 1, ([1, 2, 3], [4, 5]), hidden=16)

    def edit(fn):
        def make():
            desc = copy.deepcopy(base())
            fn(desc)
            return desc
        return make

    def repeated_af(desc):
        desc["layers"][0]["axis_af"][2] = desc["layers"][0]["axis_af"][0]

    def nn_transformed(desc):
        L = desc["layers"][0]
        L["axis_nn"][-1] = desc["n"] + L["axis_af"][0]

    def norm_bounds(desc):
        desc["layers"].append({"kind": _lib.DF_LAYER_NORM, "element": 2, "alpha": 1.0, "beta": 1.0,
                               "x_min": np.zeros(5, np.float32), "x_max": np.ones(5, np.float32)})

    def nice_with_s(desc):
        desc["layers"][1]["kind"] = _lib.DF_LAYER_NICE

    def no_chain(desc):
        D = desc["layers"][0]["t_net"][1]
        D["in"] = 12
        D["W"] = np.zeros((D["out"], 12), np.float32)

    def elements(desc):
        desc["layers"][0]["element"], desc["layers"][1]["element"] = 1, 0

    def abi(desc):
        desc["abi"] = 99

    return {
        "fail_state_65": lambda: _spec_chain(np.random.default_rng(9), 60, 5, ([1, 2],), hidden=16),
        "fail_hidden_300": lambda: _spec_chain(np.random.default_rng(9), 5, 0, ([1],), hidden=300),
        "fail_repeated_axis_af": edit(repeated_af),
        "fail_axis_nn_transformed": edit(nn_transformed),
        "fail_beta_le_alpha": edit(norm_bounds),
        "fail_nice_with_s_net": edit(nice_with_s),
        "fail_dense_in_dim": edit(no_chain),
        "fail_n_af_33": lambda: _spec_chain(np.random.default_rng(9), 40, 0, (list(range(1, 34)),), hidden=16),
        "fail_elements_decrease": edit(elements),
        "fail_abi_99": edit(abi),
    }


def matrix():
    """name: (descriptor builder, exact, environment).  Builders are cached by identity, so
    the runs that share a chain serialise it once."""
    cfg = {}

    def config(name):
        def make():
            if not cfg:
                cfg.update(_bench_configs())
            return cfg[name]
        return make

    M = {}
    for name, entry in list(E.CASES.items()) + list(E.NORM_ONLY.items()):
        env = entry[3] if name in E.CASES else {}
        M[f"edge_{name}"] = (lambda name=name: describe(spec_to_element(E.case_spec(name)).layers), -1, env)
    for c in ("cfg1", "cfg2", "cfg4"):
        M[f"{c}_auto"] = (config(c), -1, {})
        M[f"{c}_exact"] = (config(c), 1, {})
    for name in HP.MODELS:
        M[f"pin_{name}"] = (lambda name=name: describe(HP.build_model(name).layers, n_hint=HP.MODELS[name][1]), -1, {})
    M["nobias_h32"] = (_small(hidden=32, bias=False), -1, {})
    M["nobias_h256"] = (_small(hidden=256, bias=False), -1, {})
    M["n_sub_3"] = (_small(hidden=32, n_sub=3), -1, {})
    M["n_sub_1"] = (_small(hidden=32, n_sub=1), -1, {})
    M["single_dense"] = (lambda: describe(spec_to_element(_single_dense_spec(np.random.default_rng(7))).layers), -1, {})
    M["wide_first_in40"] = (_wide_first, -1, {})
    for k, v in (("DF_NO_FOLD", "1"), ("DF_NO_FAST", "1"), ("DF_FORCE_GENERIC", "1"), ("DF_SPLIT_LDS_KB", "48"),
                 ("DF_STAGE_KB", "8")):
        M[f"cfg2_{k}"] = (M["cfg2_auto"][0], -1, {k: v})
    M["edge_generic_custom_DF_STAGE_KB"] = (M["edge_generic_custom"][0], -1, {"DF_STAGE_KB": "8"})
    M["edge_wide_split_DF_NO_WIDE"] = (M["edge_wide_split"][0], -1, {"DF_NO_WIDE": "1"})
    for name, make in _failing().items():
        M[name] = (make, -1, {})
    return M


# ---------------------------------------------------------------------------
# building and running the program
# ---------------------------------------------------------------------------

def compile_program(plan_cpp, exe, sanitize=True, program="plan_fingerprint.cpp", more=()):
    """program (of this directory) with plan_cpp and the sources in more."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the planner fingerprint"
    flags = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
              "-static-libubsan"] if sanitize else ["-O2"])   # -O2: the library's own flags (--time)
    subprocess.run([cxx, "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", HERE,
                    os.path.join(HERE, program), plan_cpp, *more, "-o", exe], check=True)
    return exe


def run_matrix(exe, workdir):
    """{case: output lines} of the whole matrix."""
    M = matrix()
    files = {}
    for name, (make, _, _) in M.items():      # serial: builders share caches and seeds
        if make not in files:
            files[make] = os.path.join(workdir, f"{name}.desc")
            serialise(make(), files[make])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DF_")}

    def one(name):
        make, exact, env = M[name]
        r = subprocess.run([exe, files[make], str(exact)], capture_output=True, text=True, env=dict(clean, **env))
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout.splitlines()

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(M, pool.map(one, M)))


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("plan_fingerprint"))
    exe = compile_program(os.path.join(CSRC, "df_plan.cpp"), os.path.join(work, "plan_fingerprint"))
    return run_matrix(exe, work)


WANT = {}
if os.path.exists(GOLDEN):
    with open(GOLDEN) as _f:
        WANT = json.load(_f)


def test_expectations_are_committed():
    assert WANT, GOLDEN


def test_matrix_is_the_recorded_one():
    assert sorted(matrix()) == sorted(WANT)
    assert len([n for n in WANT if n.startswith("fail_")]) == 10
    for name, lines in WANT.items():
        refused = not lines[0].startswith("status 0")
        assert refused == name.startswith("fail_") or name == "cfg2_DF_STAGE_KB", (name, lines[0])


@pytest.mark.parametrize("name", sorted(WANT))
def test_plan_is_the_parents(got, name):
    assert got[name] == WANT[name], [(a, b) for a, b in zip(got[name], WANT[name]) if a != b]


if __name__ == "__main__":
    import tempfile

    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    with tempfile.TemporaryDirectory() as work:
        exe = compile_program(sys.argv[2], os.path.join(work, "plan_fingerprint"))
        out = run_matrix(exe, work)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", len(out), "cases from", sys.argv[2])
