"""Where a kernel's waves wait for LDS, read from its assembly (no GPU needed).

    hipcc <the Makefile's flags of the unit> -S --cuda-device-only df_uniform_ht4.hip -o ht4.s
    python tools/isa_waits.py ht4.s [--kernel REGEX]

For every kernel whose (mangled) name matches REGEX (default: the FAST SPLIT instances
uniform_kernel<4, M, true, true, true, true>) it prints the register line of the kernel
and one line per net body.  A net body is an innermost loop that holds product MFMAs
(v_mfma_f32_16x16x32_*): the tile-group loop of one (phase, output count) pair.  Per body:

  runs     product MFMAs between two waits that retire LDS reads (the run lengths)
  waits    all s_waitcnt of the body
  lgkm     those that retire at least one LDS read
  exposed  those of lgkm that retire a read issued after the last MFMA before the wait:
           nothing of the wave's own matrix work covers that read's round trip
  nop5     s_nop >= 5 directly before a ds_read (an MFMA operand overwritten too early)
  head     s_waitcnt before the body's first product MFMA: the dependent round trips
           (scalar cache or LDS) a wave makes before it has matrix work
  s_load   scalar loads inside the body (descriptor words that were not hoisted)

and per kernel the v_writelane / v_readlane moves (SGPR spills to VGPR lanes) and how many
of them lie inside a loop that holds a net body (the layer loop and everything in it).

LDS and scalar-memory operations retire in issue order for this count (the compiler
waits lgkmcnt(0) whenever a scalar load is outstanding, which the model reproduces).
"""
import argparse
import re
import sys

DEFAULT = r"uniform_kernelILi4ELi[0-3]ELb1ELb1ELb1ELb1E"
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)")
ANY_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
LANE_MOVE = re.compile(r"^\s+v_(writelane|readlane)_b32\b")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def kernels(lines):
    """(name, first line, last line) of every kernel: its label to its .Lfunc_end."""
    out, cur = [], None
    for i, ln in enumerate(lines):
        if cur is None:
            m = re.match(r"^(_Z\w+):", ln)
            if m:
                cur = (m.group(1), i)
        elif ln.startswith(".Lfunc_end"):
            out.append((cur[0], cur[1], i))
            cur = None
    return out


def stats(lines, a, b):
    """NumVgprs / ScratchSize / Occupancy comments that follow the kernel's code."""
    got = {}
    for ln in lines[b:b + 60]:
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", ln)
        if m:
            got[m.group(1)] = int(m.group(2))
    return got


def bodies(lines, a, b):
    """Innermost loops [label, backward branch] that hold a product MFMA."""
    at = {}
    loops = []
    for i in range(a, b):
        m = LABEL.match(lines[i])
        if m:
            at[m.group(1)] = i
            continue
        m = BRANCH.match(lines[i])
        if m and m.group(1) in at:
            loops.append((at[m.group(1)], i))
    inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    return [l for l in inner if any("v_mfma_f32_16x16x32" in lines[i] for i in range(l[0], l[1]))]


def lane_moves(lines, a, b, net_bodies):
    """(all v_writelane / v_readlane of the kernel, those inside a loop that holds a net body)."""
    at, loops = {}, []
    for i in range(a, b):
        m = LABEL.match(lines[i])
        if m:
            at[m.group(1)] = i
            continue
        m = ANY_BRANCH.match(lines[i])
        if m and m.group(1) in at:
            loops.append((at[m.group(1)], i))
    outer = [l for l in loops if any(l[0] <= nb[0] and nb[1] <= l[1] and l != nb for nb in net_bodies)]
    outer += list(net_bodies)
    moves = [i for i in range(a, b) if LANE_MOVE.match(lines[i])]
    inside = [i for i in moves if any(l[0] <= i <= l[1] for l in outer)]
    return len(moves), len(inside)


def head_line(lines, a, b):
    """(s_waitcnt before the first product MFMA of the body, scalar loads in the body)."""
    head, seen, s_loads = 0, False, 0
    for i in range(a, b + 1):
        ln = lines[i].split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        op = ln.split()[0]
        if op.startswith("v_mfma") and "16x16x32" in op:
            seen = True
        elif op == "s_waitcnt" and not seen:
            head += 1
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            s_loads += 1
    return head, s_loads


def body_line(lines, a, b):
    fifo = []          # outstanding lgkm operations: (is an LDS read, MFMAs issued before it)
    n_mfma = 0         # all matrix instructions so far
    run, runs = 0, []
    waits = lgkm = exposed = nop5 = 0
    prev = ""
    for i in range(a, b + 1):
        ln = lines[i].split(";")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        op = ln.split()[0]
        if op.startswith("v_mfma"):
            n_mfma += 1
            if "16x16x32" in op:
                run += 1
        elif op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
            if op.startswith("ds_read") and prev.startswith("s_nop") and int(prev.split()[1]) >= 5:
                nop5 += 1
            fifo.append((op.startswith("ds_read"), n_mfma))
        elif op == "s_waitcnt":
            waits += 1
            m = LGKM.search(ln)
            if m:
                keep = int(m.group(1))
                gone = fifo[:len(fifo) - keep] if keep else fifo
                fifo = fifo[len(fifo) - keep:] if keep else []
                reads = [g for g in gone if g[0]]
                if reads:
                    lgkm += 1
                    if any(g[1] == n_mfma for g in reads):
                        exposed += 1
                    if run:
                        runs.append(run)
                    run = 0
        prev = ln
    if run:
        runs.append(run)
    return runs, waits, lgkm, exposed, nop5


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", default=DEFAULT, help="regular expression on the mangled kernel name")
    args = ap.parse_args()
    lines = open(args.asm).read().splitlines()
    pat = re.compile(args.kernel)
    found = 0
    for name, a, b in kernels(lines):
        if not pat.search(name):
            continue
        found += 1
        s = stats(lines, a, b)
        print(f"{name}: VGPRs {s.get('NumVgprs')} scratch {s.get('ScratchSize')} occupancy {s.get('Occupancy')}")
        tot = [0, 0, 0, 0]
        heads, loads = [], 0
        net_bodies = bodies(lines, a, b)
        for k, (la, lb) in enumerate(net_bodies):
            runs, waits, lgkm, exposed, nop5 = body_line(lines, la, lb)
            head, s_loads = head_line(lines, la, lb)
            heads.append(head)
            loads += s_loads
            tot = [x + y for x, y in zip(tot, (waits, lgkm, exposed, nop5))]
            print(f"  body {k} lines {la + 1}-{lb + 1}: runs {runs} waits {waits} lgkm {lgkm} "
                  f"exposed {exposed} nop5 {nop5} head {head} s_load {s_loads}")
        print(f"  all bodies: waits {tot[0]} lgkm {tot[1]} exposed {tot[2]} nop5 {tot[3]} "
              f"head {sorted(set(heads))} s_load {loads}")
        n_moves, n_inside = lane_moves(lines, a, b, net_bodies)
        print(f"  v_writelane/v_readlane: {n_moves}, inside the layer loop: {n_inside}")
    if not found:
        print(f"no kernel matches {args.kernel}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
