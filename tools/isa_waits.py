#!/usr/bin/env python3
"""Vector-memory waits inside the loops of one kernel of a gfx950 assembly
listing (hipcc -S --cuda-device-only), set against the VMEM instructions the
loop itself has issued.

vmcnt counts outstanding vector-memory operations, oldest first: `s_waitcnt
vmcnt(N)` returns once at most N are outstanding.  A software-pipelined loop
issues this trip's loads for a LATER trip, then waits for an earlier trip's
data.  If the loop has issued k VMEM instructions since its top when it
waits, any N < k makes the wave wait for one of the loads of this same trip
and the intended load distance is lost.  (The compiler must assume the fewest
operations on any path, so a branch around a load or store lowers N.)

For each loop of the kernel (a label that a later branch jumps back to) the
tool lists every vmcnt wait between the label and that branch, in program
order, with k, and flags the waits with N < k.  Only waits and
buffer_/global_ loads and stores are read; instructions on both arms of a
branch inside the loop all count toward k, so a flag is a place to read, not
a verdict.  In a loop the compiler unrolled, k runs over all the unrolled
trips: --step-at OPCODE restarts the count at each OPCODE (k_cgs closes
every row step with s_barrier).

    python tools/isa_waits.py driver.s _Z5k_cgsILb0ELb0EEv7PcgArgsiii --step-at s_barrier
"""
import argparse
import re
import sys

_VMEM = re.compile(r"^(buffer|global)_(load|store|atomic)")
_WAIT = re.compile(r"^s_waitcnt\b.*\bvmcnt\((\d+)\)")
_LABEL = re.compile(r"^([.\w$]+):")
_BRANCH = re.compile(r"^s_c?branch\w*\s+([.\w$]+)")


def kernel_body(asm, symbol):
    """lines of `symbol:` up to its .Lfunc_end / s_endpgm-free end marker"""
    out, on = [], False
    for ln in asm.splitlines():
        t = ln.strip()
        if not on:
            on = t.split(";")[0].strip() == symbol + ":"
            continue
        if t.startswith(".Lfunc_end") or t.startswith(".end_amdhsa_kernel"):
            break
        out.append(t)
    if not out:
        raise ValueError(f"kernel {symbol} not found")
    return out


def loop_waits(lines, step_at=None):
    """[{label, start, end, waits: [{line, n, issued, short}], vmem}] for every
    backward branch; start / end / line are indices into `lines`; issued
    restarts at every instruction named step_at"""
    labels = {}
    for i, t in enumerate(lines):
        m = _LABEL.match(t)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, t in enumerate(lines):
        m = _BRANCH.match(t)
        if not m or labels.get(m.group(1), i + 1) > i:
            continue
        start, issued, total, waits = labels[m.group(1)], 0, 0, []
        for j in range(start, i):
            u = lines[j].split(";")[0].split("//")[0].strip()
            if _VMEM.match(u):
                issued += 1
                total += 1
                continue
            if step_at and u.split()[:1] == [step_at]:
                issued = 0
                continue
            w = _WAIT.match(u)
            if w:
                n = int(w.group(1))
                waits.append({"line": j, "n": n, "issued": issued, "short": n < issued})
        loops.append({"label": m.group(1), "start": start, "end": i, "waits": waits, "vmem": total})
    return loops


def report(symbol, loops, min_vmem=1):
    out = [symbol]
    for lp in loops:
        if lp["vmem"] < min_vmem:
            continue
        out.append(f"  loop {lp['label']}  ({lp['end'] - lp['start']} lines, {lp['vmem']} VMEM)")
        for w in lp["waits"]:
            out.append(f"    +{w['line'] - lp['start']:<5d} vmcnt({w['n']})  issued {w['issued']}"
                       + ("   <-- covers a load of this trip" if w["short"] else ""))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("symbol")
    ap.add_argument("--min-vmem", type=int, default=1, help="skip loops with fewer VMEM instructions")
    ap.add_argument("--step-at", default=None, metavar="OPCODE", help="restart the issued count at this opcode")
    a = ap.parse_args()
    try:
        loops = loop_waits(kernel_body(open(a.asm).read(), a.symbol), a.step_at)
    except ValueError as e:
        sys.exit(str(e))
    print(report(a.symbol, loops, a.min_vmem))


if __name__ == "__main__":
    main()
