"""What a kernel's net bodies ask of the SIMD's vector-issue port, read from its assembly
(no GPU needed): the companion of tools/isa_waits.py, with its kernels and net bodies.

    hipcc <the Makefile's flags of the unit> -S --cuda-device-only df_uniform_ht4.hip -o ht4.s
    python tools/isa_issue.py ht4.s [--kernel REGEX]

For every kernel whose (mangled) name matches REGEX (default: the eight FAST SPLIT
instances uniform_kernel<2|4, M, true, true, true, true>) it prints the kernel's VGPRs,
scratch size and occupancy and one line per net body (an innermost loop that holds product
MFMAs: the tile-group loop of one (phase, output count) pair) with the instructions of
the body by class:

  mfma     product MFMAs (v_mfma_f32_16x16x32_*)
  mfma2    2-pass MFMAs (v_mfma_f32_4x4x4_*: the split's remainders)
  valu     plain vector ALU instructions (every v_* that is none of the other classes)
  cvt      v_cvt_pk_bf16_f32
  trans    transcendentals (v_exp / v_log / v_rcp / v_rsq / v_sqrt / v_sin / v_cos)
  ds_r/w   LDS reads and writes
  nop      s_nop instructions (and the wait states they ask for, +1 each, in brackets)
  wait     s_waitcnt

and two sums from the price list of the vector-issue port (cycles an instruction holds the
port of its SIMD: MFMA 8 of the 16 or 8 its pipe is busy, plain VALU 4, conversion 4.5,
transcendental 8; costs add):

  issue    8·(mfma + mfma2) + 4·valu + 4.5·cvt + 8·trans
  pipe     16·mfma + 8·mfma2, what the matrix pipe alone needs

It only counts instruction classes: no latencies, no dependencies, no other wave.
"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import isa_waits as W  # noqa: E402

DEFAULT = r"uniform_kernelILi[24]ELi[0-3]ELb1ELb1ELb1ELb1E"
PRICE = {"mfma": 8.0, "mfma2": 8.0, "valu": 4.0, "cvt": 4.5, "trans": 8.0}
PIPE = {"mfma": 16.0, "mfma2": 8.0}
TRANS = re.compile(r"^v_(exp|log|rcp|rsq|sqrt|sin|cos)_")
CLASSES = ("mfma", "mfma2", "valu", "cvt", "trans", "ds_read", "ds_write", "s_nop", "s_waitcnt")


def classify(op):
    """The class of one mnemonic, or None for what is not counted (scalar ALU, branches...)."""
    if op.startswith("v_mfma"):
        return "mfma" if "16x16x32" in op else "mfma2"
    if op.startswith("v_cvt_pk_bf16_f32"):
        return "cvt"
    if TRANS.match(op):
        return "trans"
    if op.startswith("v_"):
        return None if op.startswith("v_nop") else "valu"
    for c in ("ds_read", "ds_write", "s_nop", "s_waitcnt"):
        if op.startswith(c):
            return c
    return None


def census(lines, a, b):
    """Instruction counts by class over lines[a..b], and the wait states of the s_nop."""
    n = dict.fromkeys(CLASSES, 0)
    states = 0
    for i in range(a, b + 1):
        ln = lines[i].split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        f = ln.split()
        c = classify(f[0])
        if c is None:
            continue
        n[c] += 1
        if c == "s_nop" and len(f) > 1:
            states += int(f[1], 0) + 1
    return n, states


def issue_cycles(n):
    return sum(PRICE[c] * n[c] for c in PRICE)


def pipe_cycles(n):
    return sum(PIPE[c] * n[c] for c in PIPE)


def report(lines, pattern, out=sys.stdout):
    pat = re.compile(pattern)
    found = 0
    for name, a, b in W.kernels(lines):
        if not pat.search(name):
            continue
        found += 1
        s = W.stats(lines, a, b)
        print(f"{name}: VGPRs {s.get('NumVgprs')} scratch {s.get('ScratchSize')} occupancy {s.get('Occupancy')}",
              file=out)
        tot = dict.fromkeys(CLASSES, 0)
        net_bodies = W.bodies(lines, a, b)
        for k, (la, lb) in enumerate(net_bodies):
            n, states = census(lines, la, lb)
            for c in CLASSES:
                tot[c] += n[c]
            print(f"  body {k} lines {la + 1}-{lb + 1}: mfma {n['mfma']} mfma2 {n['mfma2']} valu {n['valu']} "
                  f"cvt {n['cvt']} trans {n['trans']} ds_r {n['ds_read']} ds_w {n['ds_write']} "
                  f"nop {n['s_nop']} [{states}] wait {n['s_waitcnt']} issue {issue_cycles(n):.0f} "
                  f"pipe {pipe_cycles(n):.0f}", file=out)
        nb = max(len(net_bodies), 1)
        print(f"  mean of {len(net_bodies)} bodies: valu+cvt+trans {(tot['valu'] + tot['cvt'] + tot['trans']) / nb:.1f} "
              f"ds_r {tot['ds_read'] / nb:.1f} ds_w {tot['ds_write'] / nb:.1f} nop {tot['s_nop'] / nb:.1f} "
              f"wait {tot['s_waitcnt'] / nb:.1f} issue {issue_cycles(tot) / nb:.0f} pipe {pipe_cycles(tot) / nb:.0f}",
              file=out)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=DEFAULT, help="regular expression on the mangled kernel name")
    args = ap.parse_args()
    lines = open(args.asm).read().splitlines()
    if not report(lines, args.kernel):
        print(f"no kernel matches {args.kernel}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
