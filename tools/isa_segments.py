#!/usr/bin/env python3
"""Instruction classes per segment of one kernel of a gfx950 assembly listing
(hipcc -S --cuda-device-only), the listing split at every occurrence of one
opcode.

k_cgs closes every row step of every role with s_barrier, so split there a
segment is one unrolled row step of one role.  Segments are told apart by what
they issue: the key of a segment is (vector-memory instructions, LDS writes),
and --group prints one line per key with the smallest and largest count over
its segments (keys with fewer than --min-members segments, i.e. preambles and
tails, are listed as 'other').  For k_cgs<false, *> the keys are (10, 5) wave
0 (9 loads, the r store; y and the record), (0, 1) wave 1 (g1), (4, 1) wave 2
(2 loads, 2 stores; y_q), (0, 0) wave 3.

    python tools/isa_segments.py driver.s _Z5k_cgsILb0ELb0EEv7PcgArgsiii --split-at s_barrier --group
"""
import argparse
import collections
import statistics
import sys

from isa_waits import kernel_body

# counted beside the classes: the opcodes (prefix match) a row step should
# not need
WATCH = ("s_mul_hi", "s_mul_i32", "v_mov_b32", "v_cndmask", "v_rcp_f32", "v_readfirstlane", "s_cselect")
COLUMNS = ("instr", "valu", "salu", "branch", "lds", "vmem", "wait") + WATCH


def opcode(line):
    """the opcode of a listing line, or None for labels, directives, comments"""
    t = line.split(";")[0].split("//")[0].strip()
    if not t or t.endswith(":") or t.startswith("."):
        return None
    return t.split()[0]


def klass(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    return "salu"


def segments(lines, split_at):
    """[Counter] per segment in program order; the splitting instruction closes
    its segment and is counted in it"""
    out, cur = [], collections.Counter()
    for ln in lines:
        op = opcode(ln)
        if op is None:
            continue
        cur["instr"] += 1
        cur[klass(op)] += 1
        if op.startswith("ds_write"):
            cur["lds_write"] += 1
        for w in WATCH:
            if op.startswith(w):
                cur[w] += 1
        if op == split_at:
            out.append(cur)
            cur = collections.Counter()
    if cur:
        out.append(cur)
    return out


def key_of(seg):
    return seg["vmem"], seg["lds_write"]


def group(segs, min_members=6):
    """{key or 'other': {column: (min, max), 'segments': n}}"""
    by = collections.defaultdict(list)
    for s in segs:
        by[key_of(s)].append(s)
    out = {}
    for k, members in by.items():
        name = k if len(members) >= min_members else "other"
        out.setdefault(name, []).extend(members)
    return {k: dict({c: (min(s[c] for s in m), max(s[c] for s in m), int(statistics.median_low(s[c] for s in m)))
                     for c in COLUMNS}, segments=len(m))
            for k, m in out.items()}


def fmt_range(r):
    """min-max (median); the first step of a loop and its exits carry the
    loop's set-up, so the median is the steady row step"""
    return str(r[0]) if r[0] == r[1] else f"{r[0]}-{r[1]} ({r[2]})"


def table(rows):
    """rows: [(name, {column: value or (min, max)})] -> markdown"""
    out = ["| segment | " + " | ".join(COLUMNS) + " |", "|---|" + "---|" * len(COLUMNS)]
    for name, r in rows:
        out.append(f"| {name} | " + " | ".join(fmt_range(r[c]) if isinstance(r[c], tuple) else str(r[c])
                                              for c in COLUMNS) + " |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("symbol")
    ap.add_argument("--split-at", default="s_barrier", metavar="OPCODE")
    ap.add_argument("--group", action="store_true", help="one line per (VMEM, LDS writes) key, min-max")
    ap.add_argument("--min-members", type=int, default=6)
    a = ap.parse_args()
    try:
        segs = segments(kernel_body(open(a.asm).read(), a.symbol), a.split_at)
    except ValueError as e:
        sys.exit(str(e))
    print(f"{a.symbol}: {len(segs)} segments split at {a.split_at}")
    if a.group:
        g = group(segs, a.min_members)
        rows = [(f"vmem {k[0]} lds_write {k[1]} ({v['segments']} segments)" if k != "other"
                 else f"other ({v['segments']} segments)", v)
                for k, v in sorted(g.items(), key=lambda kv: (kv[0] == "other", str(kv[0])))]
    else:
        rows = [(f"{i} (vmem {s['vmem']} lds_write {s['lds_write']})", s) for i, s in enumerate(segs)]
    print(table(rows))


if __name__ == "__main__":
    main()
