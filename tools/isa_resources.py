#!/usr/bin/env python3
"""Per-kernel resources of two trees' csrc/ side by side: VGPRs, AGPRs, SGPRs, scratch bytes, static LDS, occupancy
(waves per SIMD) and instruction count of every kernel of every .hip file, compiled to gfx950 assembly with the Makefile's
flags (nn.hip with its EXTRA). Needs hipcc, no GPU.

    tools/isa_resources.py PARENT_CSRC NEW_CSRC [-j JOBS] > profiles/<name>_isa.txt

Lists every kernel whose figures differ, then the full table. Exit status 1 if a kernel gained scratch, lost occupancy
or changed its LDS. A kernel that gained a trailing template parameter whose value is `false` (a dense instantiation
beside a new twin, as profiles/ragged_tower_isa.txt) is listed under its new name against the parent's figures.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys


def makefile_flags(csrc):
    """(CXXFLAGS, {file.hip: EXTRA}) as csrc/Makefile sets them, so that the table follows the build."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    extra = {m.group(1) + ".hip": m.group(2).split() for m in re.finditer(r"^(\w+)\.o:\s*EXTRA\s*=\s*(.*)$", text, re.M)}
    return flags, extra

FIELDS = ("vgpr", "agpr", "sgpr", "scratch", "lds", "occ", "insts")
INFO = {"NumVgprs": "vgpr", "NumAgprs": "agpr", "TotalNumSgprs": "sgpr", "ScratchSize": "scratch", "LDSByteSize": "lds",
        "Occupancy": "occ"}


def kernels(path):
    path = os.path.abspath(path)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags, extra = makefile_flags(os.path.dirname(path))
    cmd = [hipcc] + flags + extra.get(os.path.basename(path), []) + ["--cuda-device-only", "-S", "-o", "-", path]
    asm = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=os.path.dirname(path)).stdout
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M))
    out = {}
    for m in re.finditer(r"^(\w+):.*?\n(.*?)^\.Lfunc_end\d+:(.*?)(?=^\s*\.(?:text|section\s+\.text|globl|protected))", asm,
                         re.M | re.S):
        name, body, tail = m.groups()
        if name not in names:
            continue
        k = {"insts": len(re.findall(r"^\s+(?:[sv]|ds|global|buffer|flat|scratch)_\w+", body, re.M))}
        for key, val in re.findall(r"^; (\w+): (\d+)", tail, re.M):
            if key in INFO:
                k[INFO[key]] = int(val)
        out[name] = k
    assert set(out) == names, (path, names - set(out))
    return out


def demangled(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True)
    short = r.stdout.split("\n") if r.returncode == 0 else names
    return dict(zip(names, short))


def parent_name(name, old):
    """The parent's name of the new kernel `name`: itself, or `name` without a trailing template argument `false`."""
    for cand in (name, re.sub(r"<false>$", "", name), re.sub(r", false>$", ">", name)):
        if cand in old:
            return cand
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a.new, "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(a.j) as ex:
        old = dict(zip(files, ex.map(lambda f: kernels(os.path.join(a.parent, f)), files)))
        new = dict(zip(files, ex.map(lambda f: kernels(os.path.join(a.new, f)), files)))
    rows, bad = [], []
    for f in files:
        short = demangled(sorted(set(old[f]) | set(new[f])))
        old_short = {short[n]: k for n, k in old[f].items()}
        twins = {parent_name(short[n], old_short) for n in new[f]}
        for n, s in short.items():
            if n in new[f]:
                o, w = old_short.get(parent_name(s, old_short)), new[f][n]
            elif s in twins:
                continue            # listed under its new name
            else:
                o, w = old[f][n], None
            rows.append((f, s, o, w))
            if o and w and (w["scratch"] > o["scratch"] or w["occ"] < o["occ"] or w["lds"] != o["lds"]):
                bad.append((f, s))
    fmt = lambda k: "-" if k is None else " ".join(f"{k.get(x, 0):>6}" for x in FIELDS)
    head = f"{'file':<22} {'':<7}" + " ".join(f"{x:>6}" for x in FIELDS) + "  kernel"
    diff = [r for r in rows if r[2] != r[3]]
    print(f"{len(rows)} kernels in {len(files)} files; {len(diff)} differ; "
          f"{len(bad)} with new scratch, lower occupancy or another LDS size")
    for title, sel in (("KERNELS THAT DIFFER", diff), ("ALL KERNELS", rows)):
        print(f"\n== {title} ==\n{head}")
        for f, s, o, w in sel:
            if o == w:
                print(f"{f:<22} {'both':<7}{fmt(o)}  {s}")
            else:
                print(f"{f:<22} {'parent':<7}{fmt(o)}  {s}\n{'':<22} {'new':<7}{fmt(w)}")
    for f, s in bad:
        print(f"CONDITION BROKEN: {f}: {s}", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
