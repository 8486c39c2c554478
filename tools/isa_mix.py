"""Static instruction mix of the MFMA-heavy basic blocks of one fused translation unit -- hipcc only, no GPU:

    python tools/isa_mix.py [neural_sim_nerf_amd/csrc/nsr_fused_h2.hip] [--kernel k_render_h2] [--min-mfma 24] [--asm FILE.s]

The unit is compiled to gfx950 assembly with the OBJFLAGS of neural_sim_nerf_amd/csrc/Makefile (about 40 s); --asm reads an
assembly file that already exists instead.  Per kernel and per basic block with at least --min-mfma MFMAs it prints
  * the number of MFMAs, VALU, v_accvgpr_* (and how many of those are v_accvgpr_mov), LDS and VMEM instructions,
  * how many instructions sit BEFORE the first and AFTER the last MFMA of the block -- with one wave per SIMD nothing covers
    them, the matrix pipe idles --, split into VALU / accvgpr / LDS / other,
  * `lead-in`: the instructions of the MFMA-free blocks that sit between the previous block holding an MFMA (or the
    kernel's entry) and this one in layout order -- the bias load of a layer ends up there when control flow splits it
    from its GEMM --, and
  * the VALU-class (VALU + v_accvgpr_*) instructions inside the last 23 MFMA gaps of the block: the shadow a GEMM's tail
    offers to the epilogue that follows it.
`outside` = before + after + lead-in is the figure tests/test_isa_mix.py holds the layer block of k_render_h2 to.
These are counts of instructions in the program text, not timings."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc")


def makefile_objflags():
    """OBJFLAGS of the csrc Makefile, $(ARCH) expanded."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^OBJFLAGS\s*=\s*(.+)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def hipcc_path():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)


def compile_to_asm(unit, out):
    cmd = [hipcc_path()] + makefile_objflags() + ["--cuda-device-only", "-S", os.path.abspath(unit), "-o", out]
    r = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise RuntimeError("%s failed with exit code %d:\n%s" % (" ".join(cmd), r.returncode, r.stderr[-4000:]))


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "acc"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    return "other"          # SALU, s_waitcnt, s_barrier, branches


def short_name(sym):
    m = re.match(r"_ZN3nsr(\d+)", sym)
    return sym[len(m.group(0)):][:int(m.group(1))] if m else sym


def parse(asm_text):
    """[(kernel, [(label, [mnemonic, ...]), ...]), ...] for every function of the assembly."""
    kernels, cur, blocks = [], None, None
    for line in asm_text.splitlines():
        s = line.strip()
        if not s or s.startswith((";", "//")):
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            lab = m.group(1)
            if lab.startswith(".LBB"):
                if blocks is not None:
                    blocks.append((lab, []))
            elif not lab.startswith("."):
                cur, blocks = lab, [("entry", [])]
                kernels.append((cur, blocks))
            continue
        if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
            blocks = None
            continue
        if s.startswith(".") or blocks is None:
            continue
        blocks[-1][1].append(s.split()[0])
    return kernels


def block_stats(ops, lead):
    cls = [classify(o) for o in ops]
    idx = [i for i, c in enumerate(cls) if c == "mfma"]
    first, last = idx[0], idx[-1]
    cnt = lambda seq: {k: sum(1 for c in seq if c == k) for k in ("valu", "acc", "lds", "vmem", "other")}
    tail_from = idx[-24] if len(idx) >= 24 else idx[0]
    tail = cls[tail_from:last]
    return dict(
        mfma=len(idx), total=cnt(cls), acc_mov=sum(1 for o in ops if o.startswith("v_accvgpr_mov")),
        before=cnt(cls[:first]), after=cnt(cls[last + 1:]), lead=cnt([classify(o) for o in lead]),
        n_before=first, n_after=len(ops) - last - 1, n_lead=len(lead),
        tail_valu=sum(1 for c in tail if c in ("valu", "acc")))


def analyse(asm_text, min_mfma=24, kernel=None):
    """{kernel: [dict(label=..., mfma=..., outside=..., ...)]} for the blocks with >= min_mfma MFMAs."""
    out = {}
    for sym, blocks in parse(asm_text):
        name = short_name(sym)
        if kernel and name != kernel:
            continue
        rows, lead = [], []
        for lab, ops in blocks:
            n = sum(1 for o in ops if classify(o) == "mfma")
            if n == 0:
                lead += ops
                continue
            if n >= min_mfma:
                st = block_stats(ops, lead)
                st["label"] = lab
                st["outside"] = st["n_before"] + st["n_after"] + st["n_lead"]
                rows.append(st)
            lead = []
        if rows:
            out[name] = rows
    return out


def fmt(d):
    return "valu %3d acc %3d lds %3d vmem %2d other %3d" % (d["valu"], d["acc"], d["lds"], d["vmem"], d["other"])


def report(res):
    lines = []
    for name in sorted(res):
        lines.append("%s" % name)
        for st in res[name]:
            lines.append("  %-12s mfma %4d | %s | accvgpr_mov %d" % (st["label"], st["mfma"], fmt(st["total"]), st["acc_mov"]))
            lines.append("  %-12s   lead-in %4d: %s" % ("", st["n_lead"], fmt(st["lead"])))
            lines.append("  %-12s   before  %4d: %s" % ("", st["n_before"], fmt(st["before"])))
            lines.append("  %-12s   after   %4d: %s" % ("", st["n_after"], fmt(st["after"])))
            lines.append("  %-12s   outside %4d   VALU-class in the last 23 MFMA gaps: %d" % ("", st["outside"], st["tail_valu"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("unit", nargs="?", default=os.path.join(CSRC, "nsr_fused_h2.hip"))
    ap.add_argument("--kernel", default=None, help="only this kernel (short name, e.g. k_render_h2)")
    ap.add_argument("--min-mfma", type=int, default=24)
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling the unit")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, "unit.s")
            compile_to_asm(a.unit, s)
            text = open(s).read()
    print("# %s, %s" % (os.path.basename(a.asm or a.unit), " ".join(makefile_objflags())))
    print(report(analyse(text, a.min_mfma, a.kernel)))


if __name__ == "__main__":
    sys.exit(main())
