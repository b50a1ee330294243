"""The repack table is closed: every packed weight blob has two writers, the host planner
(build_plan / build_train_plan, at df_chain_create, df_chain_set_weights and df_train_create)
and the device (repack() after every optimiser update, through the nine dst ← src maps of
TrainPlan::map_sources), and they must leave the same bytes.

tests/repack_closure.cpp plans one structure with two parameter sets A and B, runs A's maps on
A's blobs with B's trainables (a float copy, bf16_split_plane for plane codes 0-2, four bytes
for plane 3: what repack_kernel and repack_split_kernel do) and compares every blob byte with
B's.  It also checks every entry's bounds and alignment, that no two entries write one byte
from different sources, and that a map that is off has nothing to regather.  Each case runs
against two B's: the builder at another seed, and that B with about one parameter in eight
replaced by -0.0, +0.0, 1e-41, 2**-126, 0.5 + 2**-9 (a bf16 tie), 0.75 (exact in bf16), 3e38
(the top of the bf16 range: 0x7f62), 3.4e38 (finite in float32, rounds to bf16 inf, so the
lower planes are -inf and NaN) and NaN.

The golden fingerprints (tests/test_train_plan_fingerprint.py) pin the maps against a past
commit; this says they are right.  The program is compiled with -fsanitize=address,undefined
and run as a child process (no GPU, no code loaded into Python); DF_* variables are cleared
but for the case's own."""
import copy
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_plan_fingerprint as PF  # noqa: E402
import train_edge_cases as TE  # noqa: E402
from densityflows_amd import train as M  # noqa: E402
from helpers import _single_dense_spec, spec_to_element  # noqa: E402

MAPS = ("MP", "MT", "MW", "MWB", "MS", "MWS", "ML", "MTS", "MLS")     # TrainPlan's enum, in order
SEED_B = 4242
HOSTILE = np.array([-0.0, 0.0, 1e-41, 2.0 ** -126, 0.5 + 2.0 ** -9, 0.75, 3e38, 3.4e38, np.nan], np.float32)
MAP_LINE = re.compile(r"map (\d) (\w+) on ([01]) split ([01]) n (\d+) bytes (\d+)")


def hostile(desc, seed=99):
    """A copy of the descriptor with about one parameter in eight set to a HOSTILE value (each
    value in turn, so every one of them lands in every kind of tensor of a non-trivial chain)."""
    out = copy.deepcopy(desc)
    rng = np.random.default_rng(seed)
    k = 0
    for L in out["layers"]:
        for net in (L.get("s_net", []), L.get("t_net", [])):
            for D in net:
                for key in ("W", "b"):
                    if D[key] is None:
                        continue
                    a = np.array(D[key], np.float32, order="F")     # (describe's layout, and writable)
                    flat = a.reshape(-1, order="F")
                    hit = np.flatnonzero(rng.random(flat.shape[0]) < 0.125)
                    flat[hit] = HOSTILE[(k + np.arange(hit.shape[0])) % HOSTILE.shape[0]]
                    k += hit.shape[0]
                    D[key] = flat.reshape(a.shape, order="F") if key == "W" else flat
    assert k > 0
    return out


def matrix():
    """name: (builder of (A, B) descriptors, exact, sweep, environment).  Builders are cached by
    identity, so the cases that share a chain build and serialise it once."""
    cache = {}

    def edge(chain):
        def make():
            build = TE.EDGE_SPECS[chain][0]
            return tuple(PF.describe(spec_to_element(build(np.random.default_rng(s))).layers) for s in (0, SEED_B))
        return cache.setdefault(("edge", chain), make)

    cfg = {}

    def bench(name):
        def make():
            if not cfg:
                cfg[0], cfg[1] = PF._bench_configs(), PF._bench_configs(SEED_B)
            return cfg[0][name], cfg[1][name]
        return cache.setdefault(("bench", name), make)

    def small(**kw):
        def make():
            return PF._small(**kw)(), PF._small(seed=SEED_B, **kw)()
        return make

    def single_dense():
        return tuple(PF.describe(spec_to_element(_single_dense_spec(np.random.default_rng(s))).layers)
                     for s in (7, SEED_B))

    sweep = {k: getattr(M, "SWEEP_" + k) for k in ("AUTO", "FUSED", "H0FREE", "KEPT", "RECOMPUTE", "LAYERWISE")}
    m = {}
    for name, (chain, req, _, env) in TE.CASES.items():
        m[f"edge_{name}"] = (edge(chain), -1, sweep[req], env)
    for name in ("cfg1", "cfg2", "cfg4"):
        m[f"{name}_auto"] = (bench(name), 0, M.SWEEP_AUTO, {})
        m[f"{name}_exact"] = (bench(name), 1, M.SWEEP_AUTO, {})
    for req in ("KEPT", "RECOMPUTE", "H0FREE"):
        m[f"cfg4_{req}"] = (bench("cfg4"), 0, sweep[req], {})
    m["cfg4_AUTO_SEPARATE"] = (bench("cfg4"), 0, M.SWEEP_AUTO | M.SWEEP_SEPARATE, {})
    m["nobias_h32"] = (small(hidden=32, bias=False), 0, M.SWEEP_AUTO, {})
    m["nobias_h256"] = (small(hidden=256, bias=False), 0, M.SWEEP_AUTO, {})
    m["n_sub_1"] = (small(hidden=32, n_sub=1), 0, M.SWEEP_AUTO, {})
    m["n_sub_3"] = (small(hidden=32, n_sub=3), 0, M.SWEEP_AUTO, {})
    m["single_dense"] = (single_dense, 0, M.SWEEP_AUTO, {})
    return m


def compile_program(exe):
    return PF.compile_program(os.path.join(PF.CSRC, "df_plan.cpp"), exe, True, "repack_closure.cpp",
                              [os.path.join(PF.CSRC, "df_train_plan.cpp")])


def run_matrix(exe, workdir):
    """{(case, "seeded" | "hostile"): (return code, stdout, stderr)} of the whole matrix."""
    mat = matrix()
    files = {}
    for name, case in mat.items():      # serial: builders share caches and seeds
        if case[0] not in files:
            a, b = case[0]()
            paths = [os.path.join(workdir, f"{name}.{k}.desc") for k in ("a", "b", "h")]
            for desc, path in zip((a, b, hostile(b)), paths):
                PF.serialise(desc, path)
            files[case[0]] = paths
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DF_")}
    runs = [(name, kind) for name in mat for kind in ("seeded", "hostile")]

    def one(run):
        name, kind = run
        make, exact, sweep, env = mat[name]
        fa, fb, fh = files[make]
        r = subprocess.run([exe, fa, fb if kind == "seeded" else fh, str(exact), str(sweep)], capture_output=True,
                           text=True, env=dict(clean, **env))
        return r.returncode, r.stdout, r.stderr

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(runs, pool.map(one, runs)))


MATRIX = sorted(matrix())


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("repack_closure"))
    return run_matrix(compile_program(os.path.join(work, "repack_closure")), work)


def test_hostile_values_are_what_they_are_meant_to_be():
    """The edge values as float32 and as bf16_rne_bits (csrc/df_plan.h) rounds them."""
    bits = HOSTILE.view(np.uint32)
    assert bits[0] == 0x80000000 and bits[1] == 0
    assert 0 < bits[2] < 0x00800000 and bits[3] == 0x00800000          # a subnormal, the smallest normal
    assert bits[4] & 0xFFFF == 0x8000 and bits[5] & 0xFFFF == 0         # a tie, exact
    rne = lambda u: ((int(u) + 0x7FFF + ((int(u) >> 16) & 1)) >> 16) & 0xFFFF
    assert rne(bits[4]) == 0x3F00                                       # the tie goes to even (0.5)
    assert rne(bits[6]) == 0x7F62                                       # finite in bf16 too
    assert rne(bits[7]) == 0x7F80 and np.isfinite(HOSTILE[7])           # finite in f32, inf in bf16
    assert np.isnan(HOSTILE[8])


@pytest.mark.parametrize("kind", ["seeded", "hostile"])
@pytest.mark.parametrize("name", MATRIX)
def test_maps_are_closed(got, name, kind):
    rc, out, err = got[name, kind]
    assert rc == 0 and out.splitlines()[-1] == "closed", (name, kind, rc, out[-2000:], err[-4000:])
    assert len(MAP_LINE.findall(out)) == len(MAPS)


def test_every_map_is_on_somewhere(got):
    """A map no case switches on would go unchecked: each of the nine is on, with entries, in at
    least one case.  Prints the cases per map."""
    on = {k: [] for k in MAPS}
    for name in MATRIX:
        rc, out, _ = got[name, "seeded"]
        assert rc == 0, name
        for i, nm, flag, split, n, nbytes in MAP_LINE.findall(out):
            assert MAPS[int(i)] == nm
            assert int(split) == (nm in ("MS", "MWS", "MTS", "MLS"))
            if flag == "1" and int(n) > 0:
                assert int(nbytes) > 0
                on[nm].append(name)
    for nm in MAPS:
        print(f"REPACK MAP {nm}: on in {len(on[nm])} cases: {' '.join(on[nm])}")
    assert all(on[nm] for nm in MAPS), {nm: len(v) for nm, v in on.items()}
