"""What a net body of the specialised SPLIT kernel takes from scalar registers instead of
loading it — the layer's slot words and the offsets derived from the net's start — is
checked on the host: tests/split_head_words_check.cpp links the planner (df_plan.cpp),
plans the models of tests/golden/make_head_pin.py and config 2, and compares every word
with the table entries the kernel used to index and every offset with the planner's own.
It is compiled with -fsanitize=address,undefined and run as a child process (no GPU, no
code loaded into Python).  From its printed plan this test also checks what the pin models
are chosen for: the resident tiles (make_head_pin.MAX_TILES) and where the stage switches
fall."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_head_pin as P  # noqa: E402

CSRC = os.path.join(ROOT, "densityflows.jl_amd", "csrc")
# bench.build_chain("cfg2"): four CouplingBlocks of d = 5, cut 2 (masks [3,4,5] then [1,2]), hidden 64
CFG2 = "cfg2;5;0;64;" + ";".join(["rnvp:3,4,5", "+rnvp:1,2"] * 4)


def _arg(name):
    d, n, hidden, _, layers = P.MODELS[name]
    toks = ["norm" if k == "norm" else f"{k}:{','.join(str(v) for v in m)}" for k, m in layers]
    return ";".join([name, str(d), str(n), str(hidden)] + toks)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check"
    exe = str(tmp_path_factory.mktemp("head_words") / "split_head_words_check")
    # (the sanitizer runtimes linked in: the program runs whatever else the loader preloads)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(HERE, "split_head_words_check.cpp"), os.path.join(CSRC, "df_plan.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DF_")}  # the planner reads DF_* knobs
    r = subprocess.run([exe] + [_arg(m) for m in sorted(P.MODELS)] + [CFG2], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    out = {"models": {}, "nets": {}, "sched": {}}
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[:1] == ["model"]:
            out["models"][f[1]] = {f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}
        elif f[:1] == ["net"]:  # net NAME layer L s|t stage S off O n_out K
            out["nets"].setdefault(f[1], []).append((int(f[3]), f[4], int(f[6]), int(f[8]), int(f[10])))
        elif f[:1] == ["sched"]:
            out["sched"][f[1], f[2]] = [int(v) for v in f[3:]]
    assert r.stdout.splitlines()[-1] == "ok"
    return out


def test_words_and_offsets_match_the_tables(report):
    assert sorted(report["models"]) == sorted(list(P.MODELS) + ["cfg2"])
    assert report["models"]["cfg2"]["ht"] == 4 and len(report["nets"]["cfg2"]) == 16


@pytest.mark.parametrize("name", sorted(P.MODELS))
def test_resident_tiles_of_the_pin_models(report, name):
    assert report["models"][name]["stiles"] == P.MAX_TILES[name]


def test_where_the_stage_switches_fall(report):
    nets = report["nets"]
    # h32_ten_nets: ten nets, two per stage (the second at an offset != 0), a layer per stage
    ten = nets["h32_ten_nets"]
    assert len(ten) == 10 and report["models"]["h32_ten_nets"]["stages"] == 5
    for layer in range(5):
        (_, _, st_s, off_s, _), (_, _, st_t, off_t, _) = [x for x in ten if x[0] == layer]
        assert st_s == st_t and off_s == 0 and off_t > 0
    # h32_nice_shift: every switch but the last falls between the s- and the t-net of a layer
    shift = nets["h32_nice_shift"]
    assert len(shift) == 11
    between = [layer for layer in range(1, 6)
               if len({st for (l, _, st, _, _) in shift if l == layer}) == 2]
    assert between == [1, 2, 3, 4, 5]
    shared = [(a, b) for a, b in zip(shift, shift[1:]) if a[2] == b[2]]
    assert shared and all(a[0] != b[0] and b[3] > 0 for a, b in shared)  # two layers' nets in one stage
    # hidden 64: a stage per net
    for name in ("h64_theta_unsorted_norm", "h64_nice_first", "cfg2"):
        assert [x[2] for x in nets[name]] == list(range(len(nets[name]))), name
    # schedules: forward in packing order, backward its reverse (each stage once)
    for name in nets:
        n = report["models"][name]["stages"]
        assert report["sched"][name, "fwd"] == list(range(n))
        assert report["sched"][name, "bwd"] == list(range(n))[::-1]
