"""Kernel by kernel comparison of two device assembly files of the SAME translation unit (before / after a change that is meant to
leave the generated code alone): python tools/kernel_asm_diff.py before.s after.s [filter]

`make -C neural_sim_nerf_amd/csrc asm` writes build/<unit>_tmp-hip-amdgcn-amd-amdhsa-gfx950.s for every unit; keep the file of the
parent commit and compare.  No GPU, no compiler run.  Per kernel symbol the body is stripped of comments, .loc / .file / .cfi
lines, the numbers of temporary labels (a label is named by its first appearance in the kernel, so branch targets still compare)
and the per-build __hip_cuid_* symbol, then one verdict is printed:
  identical        the same lines in the same order
  registers only   the same lines in the same order once every v<n> / s<n> / a<n> and every register range is masked
  changed          with the opcodes whose counts differ (before -> after)
and beside it the resource lines of the kernel descriptor (.amdhsa_next_free_vgpr, _next_free_sgpr, _accum_offset,
_group_segment_fixed_size, _private_segment_fixed_size) of both sides.  A generic differ: it knows no instruction.
Exit status 1 when a kernel is changed or exists on one side only."""
import collections
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
SHORT = ("vgpr", "sgpr", "accum", "lds", "scratch")
LABEL = re.compile(r"(?<![\w.])\.L\w+")                                    # .LBB12_3, .Ltmp4, .Lfunc_end12
REG = re.compile(r"\b([vsa])(?:\d+|\[\d+:\d+\])(?![\w.])")


def kernels(path):
    """{symbol: (code lines, {resource: value})} of the .amdhsa_kernel symbols of an assembly file."""
    text = open(path).read().split("\n")
    names = [m.group(1) for line in text for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)] if m]
    out = {}
    i = 0
    while i < len(text):
        m = re.match(r"(\S+):\s*(;.*)?$", text[i])
        if not (m and m.group(1) in names and m.group(1) not in out):
            i += 1
            continue
        name, body = m.group(1), []
        i += 1
        while i < len(text) and not re.match(r"\s*\.end_amdhsa_kernel", text[i]):
            body.append(text[i])
            i += 1
        code, res, in_desc, labels = [], {}, False, {}
        for line in body:
            line = line.split(";")[0].split("//")[0].strip()
            if re.match(r"\.amdhsa_kernel\b", line):
                in_desc = True
            if in_desc:
                r = re.match(r"\.amdhsa_(\w+)\s+(\S+)", line)
                if r and r.group(1) in RESOURCES:
                    res[r.group(1)] = r.group(2)
                continue
            if not line or re.match(r"\.(loc|file|cfi_\w+|section|p2align|type|size|set|globl|protected|weak)\b", line):
                continue                                                     # debug lines, what stands in front of the descriptor
            # a temporary label's number is the build's: name it by its first appearance in the kernel, so that branches still compare
            line = LABEL.sub(lambda m: "L%d" % labels.setdefault(m.group(0), len(labels)), re.sub(r"__hip_cuid_\w+", "__hip_cuid", line))
            code.append(re.sub(r"\s+", " ", line))
        out[name] = (code, res)
    return out


def pretty(sym):
    """kw_trunk_h2<2,0,4> for _ZN4nsrw11kw_trunk_h2ILi2ELb0ELi4EEEvNS_9TrunkArgsE; other symbols as they are."""
    m = re.match(r"_ZN\d+[a-z_]+?(\d+)", sym)
    if not m:
        return sym
    rest = sym[m.end():]
    base, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
    t = re.match(r"I((?:L[ibjlm]\d+E)+)E", rest)
    return base + ("<%s>" % ",".join(re.findall(r"L[ibjlm](\d+)E", t.group(1))) if t else "")


def opcode_diff(a, b):
    ca, cb = (collections.Counter(line.split(" ")[0] for line in x if not line.endswith(":")) for x in (a, b))
    return ["%s %d -> %d" % (op, ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]]


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    a, b = kernels(argv[1]), kernels(argv[2])
    want = argv[3] if len(argv) > 3 else ""
    tally, bad = collections.Counter(), False
    print("%-34s %-15s %6s %6s   %s" % ("kernel", "verdict", "lines", "", " ".join("%s" % s for s in SHORT)))
    for sym in sorted(set(a) | set(b), key=pretty):
        if want not in pretty(sym) and want not in sym:
            continue
        if sym not in a or sym not in b:
            print("%-34s %-15s" % (pretty(sym), "only in " + ("before" if sym in a else "after")))
            bad = True
            continue
        (ca, ra), (cb, rb) = a[sym], b[sym]
        mask = lambda code: [REG.sub(r"\1#", line) for line in code]
        verdict = "identical" if ca == cb else "registers only" if mask(ca) == mask(cb) else "changed"
        tally[verdict] += 1
        bad |= verdict == "changed"
        res = " ".join(ra.get(k, "-") if ra.get(k) == rb.get(k) else "%s->%s" % (ra.get(k, "-"), rb.get(k, "-")) for k in RESOURCES)
        print("%-34s %-15s %6d %6d   %s" % (pretty(sym), verdict, len(ca), len(cb), res))
        if verdict == "changed":
            for d in opcode_diff(ca, cb) or ["the same opcode counts: another order, or other operands"]:
                print("    " + d)
    print(", ".join("%d %s" % (n, v) for v, n in sorted(tally.items())))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
