"""Resource usage of every painter instantiation (k_paint_wave / _quad / _deep / _huge), from the compiler's
-Rpass-analysis=kernel-resource-usage remarks, plus a hash of each kernel's gfx950 ISA.  No GPU needed.

    python tools/paint_remarks.py                     # the working tree
    python tools/paint_remarks.py --rev HEAD~1        # paint.hip and its headers as of a git revision
    python tools/paint_remarks.py --rev A --compare   # A against the working tree: the SRGB8 painters must be identical

Kernels are keyed by their demangled name; the output-format template argument (FMT, last) is split off, so the SRGB8
instantiations of a tree with FMT line up with the same painters of a tree without it.  The ISA hash is taken over the kernel's
instructions with its own symbol names removed."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "forma_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-fno-fast-math", "-fno-gpu-flush-denormals-to-zero", '-DFORMA_ARCH="gfx950"', "--cuda-device-only"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # (as forma_amd/csrc/Makefile)
PAINTERS = ("k_paint_wave", "k_paint_quad", "k_paint_deep", "k_paint_huge")
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill",
          "LDS Size [bytes/block]": "lds"}


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def _key(demangled):
    """'void k_paint_wave<true, true, 4, 0>(...)' -> ('k_paint_wave<true, true, 4>', 'srgb8'); no FMT argument -> 'srgb8'"""
    sig = re.sub(r"^void ", "", demangled.split("(")[0])
    m = re.match(r"(\w+)(?:<(.*)>)?$", sig)
    name, args = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    base_n = {"k_paint_wave": 3, "k_paint_quad": 1, "k_paint_deep": 2, "k_paint_huge": 0}[name]
    fmt = "srgb8"
    if len(args) > base_n:
        fmt = {"0": "srgb8", "1": "linear_f16"}[args[base_n]]
        args = args[:base_n]
    return (name + ("<" + ", ".join(args) + ">" if args else "")), fmt


def collect(src_dir):
    tmp = tempfile.mkdtemp(prefix="paint_remarks_")
    try:
        asm = os.path.join(tmp, "paint.s")
        r = subprocess.run([HIPCC] + FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-S",
                            os.path.join(src_dir, "paint.hip"), "-o", asm], capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        kern, res = None, {}
        for line in r.stderr.splitlines():
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                kern = m.group(1); res[kern] = {}
                continue
            m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
            if m and kern and m.group(1) in FIELDS:
                v = m.group(2)
                res[kern][FIELDS[m.group(1)]] = v if v in ("True", "False") else int(v)
        text = open(asm).read()
        isa = {}
        for k in res:                                   # the kernel's body: from its label to its .Lfunc_end
            m = re.search(r"^" + re.escape(k) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M)
            body = m.group(1) if m else ""
            # (a template kernel lives in a COMDAT section of its own: section directives are not code)
            body = "\n".join(l.split(";")[0].rstrip() for l in body.splitlines()
                             if l.strip() and not l.lstrip().startswith((";", ".section", ".text")))
            body = body.replace(k, "KERNEL")
            body = re.sub(r"\.LBB\d+_", ".LBB_", body)   # (block labels are numbered per file)
            isa[k] = hashlib.sha1(body.encode()).hexdigest()[:16]
        names = _demangle(list(res))
        out = {}
        for k, v in res.items():
            d = names[k]
            if not any(p in d for p in PAINTERS):
                continue
            name, fmt = _key(d)
            v["isa_sha1"] = isa[k]
            out.setdefault(name, {})[fmt] = v
        return {k: out[k] for k in sorted(out)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def tree_at(rev):
    d = tempfile.mkdtemp(prefix="paint_rev_")
    for sub in ("forma_amd/csrc", "include"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    files = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", rev, "forma_amd/csrc/", "include/"],
                           capture_output=True, text=True, check=True).stdout.split()
    for f in files:
        with open(os.path.join(d, f), "wb") as fh:
            fh.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{f}"], capture_output=True, check=True).stdout)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default=None, help="git revision to compile instead of the working tree")
    ap.add_argument("--compare", action="store_true", help="--rev against the working tree; exit 1 if an SRGB8 painter differs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rev:
        d = tree_at(a.rev)
        try:
            before = collect(os.path.join(d, "forma_amd", "csrc"))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    else:
        before = None
    if a.compare:
        after = collect(CSRC)
        diff = [k for k in before if before[k].get("srgb8") != after.get(k, {}).get("srgb8")]
        missing = [k for k in before if k not in after]
        res = {"rev": a.rev, "before": before, "after": after, "srgb8_identical": not diff and not missing,
               "srgb8_differs": diff + missing}
    else:
        res = before if before is not None else collect(CSRC)
    js = json.dumps(res, indent=1)
    if a.out:
        open(a.out, "w").write(js + "\n")
    print(js if not a.compare else json.dumps({"srgb8_identical": res["srgb8_identical"], "srgb8_differs": res["srgb8_differs"]}))
    if a.compare and not res["srgb8_identical"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
