#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two source trees (CPU only: a cross-compile, no GPU, no network).

    tools/isa_compare.py PARENT_TREE NEW_TREE mvsn_chain_wino.hip mvsn_tower.hip ...

Each tree is a checkout of this repository.  Every listed file of multi_view_stereonet_amd/csrc is compiled in both
trees with the library's own flags (build.py: HIPCC_FLAGS, + MVSN_HIPCC_FLAGS) plus `-S --cuda-device-only`; the
assembly is split per function symbol (instruction text, the .amdhsa_kernel block, the resource summary) and compared
after normalising what moves without the code moving: the function index in basic-block / function-end labels
(BB<n>_, .Lfunc_end<n>: the order of emission), runs of white space, the __hip_cuid_* symbol.  Per symbol one line:

    identical|DIFFERENT  <file>  <symbol>  [lines; mfma; vgpr; sgpr_spill; vgpr_spill; scratch]

lines = instruction lines, mfma = v_mfma among them, the rest from the kernel's amdhsa.kernels metadata entry (scratch =
.private_segment_fixed_size, bytes).  A DIFFERENT symbol prints the figures of both sides.  Exit status 1 if any symbol
differs or exists on one side only.

Kernels that changed files: the parent's files, then `--pooled` and the new tree's files; the symbols of each side are
pooled, compared by name, and a line names both files (`<parent file> -> <new file>`):

    tools/isa_compare.py PARENT_TREE NEW_TREE mvsn_conv.hip mvsn_misc.hip --pooled mvsn_conv.hip mvsn_misc.hip mvsn_groupnorm.hip"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multi_view_stereonet_amd.build import HIPCC_FLAGS, hipcc  # noqa: E402

META_KEYS = (("vgpr", ".vgpr_count"), ("sgpr_spill", ".sgpr_spill_count"), ("vgpr_spill", ".vgpr_spill_count"),
             ("scratch", ".private_segment_fixed_size"))


def compile_asm(tree, name, out):
    src = os.path.join(tree, "multi_view_stereonet_amd", "csrc", name)
    cmd = [hipcc()] + HIPCC_FLAGS + os.environ.get("MVSN_HIPCC_FLAGS", "").split() + \
        ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", src, "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), p.stdout.decode()))
    with open(out) as f:
        return f.read()


def normalise(line):
    line = re.sub(r"(?:\.L|\b)BB\d+_", "BB_", line)      # (.LBB<n>_<k> in code, BB<n>_<k> in comments)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)
    return " ".join(line.split())


def split_symbols(asm):
    """symbol -> {"text": normalised lines from its `.type sym,@function` to the next function (or the file's tail),
    "lines": instruction lines, "mfma": v_mfma among them, + the metadata figures}"""
    lines = asm.split("\n")
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"\s*\.type\s+(\S+),@function", l)] if m]
    tail = next((i for i, l in enumerate(lines) if ".AMDGPU.gpr_maximums" in l or re.match(r"\s*\.type\s+__hip_cuid", l)),
                len(lines))
    syms = {}
    for n, (i, sym) in enumerate(starts):
        end = starts[n + 1][0] if n + 1 < len(starts) else tail
        body = [normalise(l) for l in lines[i:end]]
        body = [l for l in body if l and not l.startswith("; -- Begin function") and not l.startswith(".protected")
                and not l.startswith(".globl") and not l.startswith(".p2align")
                and not l.startswith(".fill")]       # (.fill: the code-end padding behind the file's LAST function)
        while body and (body[-1] == ".text" or body[-1].startswith(".section .text")):
            body.pop()                               # the directive that opens the NEXT function's section
        code_end = next((k for k, l in enumerate(body) if l.startswith(".Lfunc_end") or l.startswith(".amdhsa_kernel")
                         or l.startswith(".section")), len(body))
        insn = [l for l in body[:code_end] if not l.startswith((";", ".")) and not re.match(r"\S+:( ;.*)?$", l)]
        syms[sym] = {"text": body, "lines": len(insn), "mfma": sum(1 for l in insn if l.startswith("v_mfma"))}
    meta = asm[asm.find("amdhsa.kernels:"):]
    meta = re.split(r"\namdhsa\.\w+:", meta)[0]      # (the keys behind the list are the file's, not the last kernel's)
    for entry in re.split(r"\n  - ", meta)[1:]:
        entry = "    " + entry
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if not name or name.group(1) not in syms:
            continue
        for key, field in META_KEYS:
            m = re.search(r"^    \%s:\s+(\d+)" % field, entry, re.M)
            syms[name.group(1)][key] = int(m.group(1)) if m else None
        # the whole entry takes part in the comparison (argument layout, LDS, kernarg size)
        syms[name.group(1)]["text"] += [normalise(l) for l in entry.split("\n") if l.strip()]
    return syms


def figures(s):
    return "%d lines; %d mfma; " % (s["lines"], s["mfma"]) + "; ".join("%s %s" % (k, s.get(k)) for k, _ in META_KEYS)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+", help=".hip files of multi_view_stereonet_amd/csrc")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--pooled", nargs="+", metavar="FILE", help="kernels may have changed files: `files` are the parent's, "
                    "these the new tree's; the symbols of each side are pooled and compared by name")
    a = ap.parse_args()
    files = {"parent": a.files, "new": a.pooled or a.files}
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {(side, f): pool.submit(compile_asm, tree, f, os.path.join(tmp, "%s_%s.s" % (side, f)))
                for side, tree in (("parent", a.parent), ("new", a.new)) for f in files[side]}
        asm = {k: split_symbols(j.result()) for k, j in jobs.items()}
    print("# flags: %s -S --cuda-device-only" % " ".join(HIPCC_FLAGS + os.environ.get("MVSN_HIPCC_FLAGS", "").split()))
    bad = 0
    if a.pooled:
        old, new = ({sym: (f, s) for f in files[side] for sym, s in asm[(side, f)].items()} for side in ("parent", "new"))
        for side, pool_ in (("parent", old), ("new", new)):
            twice = sum(len(asm[(side, f)]) for f in files[side]) - len(pool_)
            bad += twice                                 # (a kernel defined in two files of one side has no one counterpart)
            print("# %s: %s: %d symbols%s" % (side, " ".join(files[side]), len(pool_), ", %d defined twice" % twice if twice else ""))
        only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        print("# only in parent: %s; only in new: %s" % (", ".join(only_old) or "none", ", ".join(only_new) or "none"))
        bad += len(only_old) + len(only_new)
        for sym in sorted(set(old) & set(new)):
            (fo, so), (fn, sn) = old[sym], new[sym]
            if so["text"] == sn["text"]:
                print("identical  %s -> %s  %s  [%s]" % (fo, fn, sym, figures(so)))
            else:
                bad += 1
                print("DIFFERENT  %s -> %s  %s  parent [%s]  new [%s]" % (fo, fn, sym, figures(so), figures(sn)))
    for f in [] if a.pooled else a.files:
        old, new = asm[("parent", f)], asm[("new", f)]
        only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        print("# %s: symbols parent %d, new %d; only in parent: %s; only in new: %s" %
              (f, len(old), len(new), ", ".join(only_old) or "none", ", ".join(only_new) or "none"))
        bad += len(only_old) + len(only_new)
        for sym in sorted(set(old) & set(new)):
            if old[sym]["text"] == new[sym]["text"]:
                print("identical  %s  %s  [%s]" % (f, sym, figures(old[sym])))
            else:
                bad += 1
                print("DIFFERENT  %s  %s  parent [%s]  new [%s]" % (f, sym, figures(old[sym]), figures(new[sym])))
    print("# %s" % ("every symbol identical" if not bad else "%d symbols differ or are unmatched" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
