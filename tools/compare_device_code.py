#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel (no GPU needed).

    python tools/compare_device_code.py PARENT_CSRC BRANCH_CSRC [--prof] [--jobs N] > table.md

Every *.hip of both csrc directories is compiled to device assembly with the Makefile's flags (--prof: those of `make prof`).
A function is identified by its symbol, whichever file defines it, so code may move between translation units.  Per symbol
two things are compared: the instruction stream (comments dropped, the function number in basic-block labels normalised) and,
for kernels, VGPRs, SGPRs, scratch bytes, static LDS and the spill counts.  Exit status 1 if a parent symbol is missing in
the branch or differs.  A refactoring aid, not part of the test suite.
"""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EXTRA = {"scp_qp_persist": ["-fno-honor-nans"], "scp_qp_persist16": ["-fno-honor-nans"]}  # EXTRA_* of the Makefile


def compile_asm(src, out, prof):
    src = os.path.abspath(src)
    stem = os.path.splitext(os.path.basename(src))[0]
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(src)))), "include")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-w", "-I" + include,
           "-I" + os.path.dirname(os.path.abspath(src))] + EXTRA.get(stem, []) + (["-DSCP_PHASE_PROFILE"] if prof else [])
    subprocess.run(cmd + ["--cuda-device-only", "-S", src, "-o", out], check=True, cwd=os.path.dirname(os.path.abspath(src)))
    return out


LABEL = re.compile(r"\.L(BB|JTI|tmp|func_begin|func_end)(\d+)(_\d+)?")


def parse(asm_path):
    """symbol -> (stream hash, instruction count, metadata dict or None)"""
    funcs, meta, spills = {}, {}, {}
    name, body = None, []
    lines = open(asm_path).read().split("\n")
    for i, line in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*(;.*)?$", line)
        if m and not line.startswith(".L") and name is None and any(
                lines[j].startswith("\t.type\t" + m.group(1) + ",@function") for j in range(max(0, i - 6), i)):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                funcs[name] = body
                name = None
                continue
            code = line.split(";")[0].rstrip()
            if not code.strip() or code.lstrip().startswith((".p2align", ".loc", ".file", ".cfi")):
                continue
            body.append(LABEL.sub(lambda g: ".L" + g.group(1) + (g.group(3) or ""), code.strip()))
    text = "\n".join(lines)
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        meta[m.group(1)] = {"vgpr": d.get("next_free_vgpr"), "sgpr": d.get("next_free_sgpr"),
                            "scratch": d.get("private_segment_fixed_size"), "lds": d.get("group_segment_fixed_size")}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.wavefront_size:", text):
        blk = m.group(0)
        s = re.search(r"\.sgpr_spill_count:\s+(\d+)", blk)
        v = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        spills[m.group(1)] = (s.group(1) if s else "?", v.group(1) if v else "?")
    out = {}
    for n, b in funcs.items():
        md = meta.get(n)
        if md is not None:
            md = dict(md, sgpr_spill=spills.get(n, ("?", "?"))[0], vgpr_spill=spills.get(n, ("?", "?"))[1])
        out[n] = (hashlib.sha256("\n".join(b).encode()).hexdigest()[:12], len(b), md)
    return out


def tree(csrc, prof, jobs, tmp, tag):
    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        asms = list(ex.map(lambda s: compile_asm(s, os.path.join(tmp, tag + "_" + os.path.basename(s) + ".s"), prof), srcs))
    syms = {}
    for src, asm in zip(srcs, asms):
        for n, v in parse(asm).items():
            syms.setdefault(n, (os.path.basename(src),) + v)
    return syms


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        return {n: n for n in names}
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split("\n"))) if r.returncode == 0 else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        P = tree(a.parent, a.prof, a.jobs, tmp, "parent")
        B = tree(a.branch, a.prof, a.jobs, tmp, "branch")
    dm = demangle(sorted(set(P) | set(B)))
    bad = 0
    print(f"build: {'make prof (-DSCP_PHASE_PROFILE)' if a.prof else 'make all'}; parent: {len(P)} device functions, "
          f"branch: {len(B)}\n")
    print("| kernel | parent file | branch file | instr. | VGPR | SGPR | scratch B | LDS B | spills s/v | stream | metadata |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for n in sorted(P, key=lambda n: (P[n][0], dm[n])):
        pf, ph, pn, pm = P[n]
        if n not in B:
            print(f"| `{dm[n]}` | {pf} | MISSING | {pn} | | | | | | | |")
            bad += 1
            continue
        bf, bh, bn, bm = B[n]
        same_s, same_m = ph == bh, pm == bm
        bad += (not same_s) + (not same_m)
        if pm is None:  # a device function that was not inlined
            print(f"| `{dm[n]}` (function) | {pf} | {bf} | {pn} | | | | | | {'same' if same_s else 'DIFFERENT'} | |")
            continue
        print(f"| `{dm[n]}` | {pf} | {bf} | {pn} | {pm['vgpr']} | {pm['sgpr']} | {pm['scratch']} | {pm['lds']} | "
              f"{pm['sgpr_spill']}/{pm['vgpr_spill']} | {'same' if same_s else 'DIFFERENT (%d instr.)' % bn} | "
              f"{'same' if same_m else 'DIFFERENT ' + str(bm)} |")
    extra = sorted(set(B) - set(P))
    print(f"\nonly in the branch: {', '.join('`' + dm[n] + '`' for n in extra) if extra else 'none'}")
    kernels = [n for n in extra if B[n][3] is not None]
    if kernels:  # the resources of the kernels the branch adds
        print("\n| new kernel | file | instr. | VGPR | SGPR | scratch B | LDS B | spills s/v |")
        print("|---|---|---|---|---|---|---|---|")
        for n in kernels:
            bf, _, bn, bm = B[n]
            print(f"| `{dm[n]}` | {bf} | {bn} | {bm['vgpr']} | {bm['sgpr']} | {bm['scratch']} | {bm['lds']} | "
                  f"{bm['sgpr_spill']}/{bm['vgpr_spill']} |")
    print(f"\n{len(P)} parent functions compared, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
