"""The trainer's host plan, byte for byte: tests/train_plan_fingerprint.cpp links df_plan.cpp
and df_train_plan.cpp, plans one serialised chain descriptor, builds the df::TrainPlan of one
(exact, sweep request, rule list) and prints every scalar of it, a hash of every vector, every
GNet, every layer-wise Dense with both operands, and the repack table's sources (or the status
and message of a refusal).  This test runs the matrix below and compares every line with
tests/golden/train_plan_fingerprint.json (each distinct line once, and per case the indices of
its lines: _write_golden).

The expectations were recorded from the code of commit 484469a, BEFORE df_train_plan.cpp
existed: a one-off program (kept out of the tree) #included that commit's df_train_capi.hip
verbatim, defined set_err / hip_err / last_error / use_split / use_wsplit itself, filled a
host-only df_chain (plan from build_plan, exact, no_wide) and a df_train, and ran the host
statements of that commit's df_train_create_opt in their order: check_rules, the form checks,
tensor_table, build_nets / the nine clears / build_lnets, fmode_eligible, the two form
refusals and the block loop of setup_chain.  It copied the fields into a struct with
TrainPlan's member names and #included tests/train_plan_fingerprint.cpp (with
DF_TRAIN_PLAN_GIVEN) for main() and the printing code.  Compiled with `hipcc
--cuda-host-only -c`, linked with that commit's df_plan.o and
-Wl,--unresolved-symbols=ignore-all (no kernel launcher is ever called), then

    python tests/test_train_plan_fingerprint.py --record <that program>

Regenerate only for a change MEANT to alter a trainer blob, a repack map, a descriptor or an
error, from the code BEFORE that change plus a reasoned diff, never from the code under test.

The program is compiled with -fsanitize=address,undefined and run as a child process (no
GPU, no code loaded into Python); DF_* variables are cleared but for the case's own."""
import json
import os
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
from densityflows_amd import _lib  # noqa: E402
from densityflows_amd import train as M  # noqa: E402
from helpers import _single_dense_spec, spec_to_element  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "train_plan_fingerprint.json")

ADAM = (_lib.DF_OPT_ADAM, 1e-3, 0.9, 0.999, 1e-8)      # df_train_create's default
DESCENT = (_lib.DF_OPT_DESCENT, 0.01)
CLIP_GRAD = (_lib.DF_OPT_CLIP_GRAD, 0.5)
CLIP_NORM = (_lib.DF_OPT_CLIP_NORM, 1.0)
DECAY = (_lib.DF_OPT_WEIGHT_DECAY, 1e-4)

RULES_OK = {"adam": [ADAM], "clipnorm_adam": [CLIP_NORM, ADAM], "decay_clipgrad_descent": [DECAY, CLIP_GRAD, DESCENT],
            "clipgrad_clipnorm_decay_adam": [CLIP_GRAD, CLIP_NORM, DECAY, ADAM]}
RULES_REFUSED = {"none": [], "nine": [CLIP_GRAD] * 8 + [ADAM], "two_adams": [ADAM, ADAM],
                 "clipnorm_after_adam": [ADAM, CLIP_NORM], "no_terminal": [CLIP_GRAD, DECAY],
                 "negative_eta": [(_lib.DF_OPT_ADAM, -1e-3, 0.9, 0.999, 1e-8)],
                 "clipgrad_zero": [(_lib.DF_OPT_CLIP_GRAD, 0.0), ADAM], "unknown_kind": [(9, 1.0), ADAM]}
N_REFUSED = 6 + len(RULES_REFUSED)


def _rules_arg(rules):
    return "/".join(f"{r[0]}:" + ",".join(repr(float(p)) for p in r[1:]) for r in rules) or "-"


def matrix():
    """name: (descriptor builder, exact, sweep, rules, environment).  Builders are cached by
    identity, so the runs that share a chain serialise it once."""
    cache = {}

    def edge(chain):
        def make():
            return PF.describe(spec_to_element(TE.EDGE_SPECS[chain][0](np.random.default_rng(0))).layers)
        return cache.setdefault(("edge", chain), make)

    cfg = {}

    def bench(name):
        def make():
            if not cfg:
                cfg.update(PF._bench_configs())
            return cfg[name]
        return cache.setdefault(("bench", name), make)

    sweep = {k: getattr(M, "SWEEP_" + k) for k in ("AUTO", "FUSED", "H0FREE", "KEPT", "RECOMPUTE", "LAYERWISE")}
    SEP = M.SWEEP_SEPARATE
    m = {}
    for name, (chain, req, _, env) in TE.CASES.items():
        m[f"edge_{name}"] = (edge(chain), -1, sweep[req], [ADAM], env)
    for name, make in (("cfg5", edge("cfg5")), ("cfg5_in40", edge("cfg5_in40")), ("cfg1", bench("cfg1")),
                       ("cfg2", bench("cfg2")), ("cfg4", bench("cfg4"))):
        m[f"{name}_auto"] = (make, 0, M.SWEEP_AUTO, [ADAM], {})
        m[f"{name}_exact"] = (make, 1, M.SWEEP_AUTO, [ADAM], {})
    m["cfg4_AUTO_SEPARATE"] = (bench("cfg4"), 0, M.SWEEP_AUTO | SEP, [ADAM], {})
    for req in ("H0FREE", "KEPT", "RECOMPUTE", "LAYERWISE"):
        m[f"cfg4_{req}"] = (bench("cfg4"), 0, sweep[req], [ADAM], {})
        m[f"cfg4_{req}_SEPARATE"] = (bench("cfg4"), 0, sweep[req] | SEP, [ADAM], {})
    small = {"nobias_h32": PF._small(hidden=32, bias=False), "nobias_h256": PF._small(hidden=256, bias=False),
             "n_sub_3": PF._small(hidden=32, n_sub=3), "n_sub_1": PF._small(hidden=32, n_sub=1),
             "single_dense": lambda: PF.describe(spec_to_element(_single_dense_spec(np.random.default_rng(7))).layers)}
    for name, make in small.items():
        m[name] = (make, 0, M.SWEEP_AUTO, [ADAM], {})
    readme = edge("readme")
    m["refuse_fused_n_sub_3"] = (small["n_sub_3"], 0, M.SWEEP_FUSED, [ADAM], {})
    m["refuse_fused_hidden_256"] = (bench("cfg4"), 0, M.SWEEP_FUSED, [ADAM], {})
    m["refuse_fused_separate"] = (bench("cfg4"), 0, M.SWEEP_FUSED | SEP, [ADAM], {})
    m["refuse_h0free_readme"] = (readme, 0, M.SWEEP_H0FREE, [ADAM], {})
    m["refuse_kept_uniform"] = (bench("cfg2"), 0, M.SWEEP_KEPT, [ADAM], {})
    m["refuse_unknown_form"] = (readme, 0, 6, [ADAM], {})
    for name, rules in RULES_OK.items():
        m[f"rules_{name}"] = (readme, 0, M.SWEEP_AUTO, rules, {})
    for name, rules in RULES_REFUSED.items():
        m[f"refuse_rules_{name}"] = (readme, 0, M.SWEEP_AUTO, rules, {})
    return m


def compile_program(exe, sanitize=True):
    return PF.compile_program(os.path.join(PF.CSRC, "df_plan.cpp"), exe, sanitize, "train_plan_fingerprint.cpp",
                              [os.path.join(PF.CSRC, "df_train_plan.cpp")])


def run_matrix(exe, workdir):
    """{case: output lines} of the whole matrix."""
    mat = matrix()
    files = {}
    for name, case in mat.items():      # serial: builders share caches and seeds
        if case[0] not in files:
            files[case[0]] = os.path.join(workdir, f"{name}.desc")
            PF.serialise(case[0](), files[case[0]])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("DF_")}

    def one(name):
        make, exact, sweep, rules, env = mat[name]
        r = subprocess.run([exe, files[make], str(exact), str(sweep), _rules_arg(rules)], capture_output=True,
                           text=True, env=dict(clean, **env))
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout.splitlines()

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(mat, pool.map(one, mat)))


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("train_plan_fingerprint"))
    return run_matrix(compile_program(os.path.join(work, "train_plan_fingerprint")), work)


def _write_golden(out):
    """Most lines recur from case to case (the Dense lines of the config-4 sweeps, the rules of
    every plain-Adam trainer): the file holds each distinct line once, and per case the indices
    of its lines."""
    lines = sorted({l for v in out.values() for l in v})
    at = {l: i for i, l in enumerate(lines)}
    cases = [f"{json.dumps(n)}: {json.dumps([at[l] for l in out[n]], separators=(',', ':'))}" for n in sorted(out)]
    with open(GOLDEN, "w") as f:
        f.write('{"lines": [\n' + ",\n".join(json.dumps(l) for l in lines) + '\n],\n"cases": {\n'
                + ",\n".join(cases) + "\n}}\n")


WANT = {}
if os.path.exists(GOLDEN):
    with open(GOLDEN) as _f:
        _g = json.load(_f)
    WANT = {n: [_g["lines"][i] for i in idx] for n, idx in _g["cases"].items()}


def test_expectations_are_committed():
    assert WANT, GOLDEN


def test_matrix_is_the_recorded_one():
    assert sorted(matrix()) == sorted(WANT)
    assert len([n for n in WANT if n.startswith("refuse_")]) == N_REFUSED == 14
    for name, lines in WANT.items():
        assert (not lines[0].startswith("status 0")) == name.startswith("refuse_"), (name, lines[0])
    for name, (_, _, form, _) in TE.CASES.items():    # each case plans the sweep it must run
        lines = WANT[f"edge_{name}"]
        assert ("layerwise 1" in lines) == (form != "FUSED"), name
        assert ("fmode 1" in lines) == (form == "H0FREE"), name


@pytest.mark.parametrize("name", sorted(WANT))
def test_train_plan_is_the_parents(got, name):
    assert got[name] == WANT[name], [(a, b) for a, b in zip(got[name], WANT[name]) if a != b]


if __name__ == "__main__":
    import tempfile

    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    with tempfile.TemporaryDirectory() as work:
        out = run_matrix(sys.argv[2], work)
    _write_golden(out)
    print("recorded", len(out), "cases from", sys.argv[2])
