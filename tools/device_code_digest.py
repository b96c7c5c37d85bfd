#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 device code in built objects or libraries; needs no GPU.

    tools/device_code_digest.py pda_amd/csrc/libpda_hip.so                  the table of one file
    tools/device_code_digest.py old/libpda_hip.so pda_amd/csrc/libpda_hip.so   both tables' differences; exit status 1 if any

For every input (.o or .so) the .hip_fatbin section is dumped (objcopy), every offload bundle in it -- a library holds one per translation
unit -- is unbundled for hipv4-amdgcn-amd-amdhsa--gfx950 (clang-offload-bundler) and disassembled (llvm-objdump -d --no-show-raw-insn).
Per kernel: name, code size, SHA-256 of its disassembly with addresses and comments stripped, and from the note metadata .vgpr_count,
.agpr_count, .sgpr_count, .private_segment_fixed_size (scratch) and .group_segment_fixed_size (static LDS).  The kernels of this library
contain no s_getpc and no calls, so where a kernel sits in its code object plays no part in its text: equal digests = the same
instructions.  The tool hashes and compares; it looks for nothing in particular.
"""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def llvm_bin():
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    return os.path.join(root, "llvm", "bin")


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stdout


def code_objects(path, tmp):
    """The gfx950 code objects of one built file, one per offload bundle, in file order."""
    fat = os.path.join(tmp, "fatbin")
    run(os.path.join(llvm_bin(), "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(tmp, "unused"))
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    if not starts:
        sys.exit(f"{path}: no offload bundle in .hip_fatbin")
    out = []
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        bundle, co = os.path.join(tmp, f"bundle{n}"), os.path.join(tmp, f"co{n}")
        open(bundle, "wb").write(blob[a:b])
        run(os.path.join(llvm_bin(), "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + co)
        if os.path.getsize(co) > 0:
            out.append(co)
    return out


def kernel_meta(co):
    """name -> the META figures, from the code object's AMDGPU note."""
    text = run(os.path.join(llvm_bin(), "llvm-readelf"), "--notes", co).decode()
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"\s*(-\s+)?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) and len(line) - len(line.lstrip()) <= 2:          # "  - .first_key:" opens a kernel's entry
            cur = {}
        if cur is None:
            continue
        key, val = m.group(2), m.group(3).strip().strip("'\"")
        if key in META:
            cur[key] = int(val)
        elif key == ".name":
            kernels[val] = cur
    return kernels


def functions(co):
    """name -> (size in bytes, sha256 of the stripped disassembly), for every function symbol of the code object."""
    sizes = {}
    for line in run(os.path.join(llvm_bin(), "llvm-readelf"), "-sW", co).decode().splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            sizes[f[7]] = int(f[2], 0)
    text = run(os.path.join(llvm_bin(), "llvm-objdump"), "-d", "--no-show-raw-insn", co).decode()
    out, name, h = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if name is not None:
                out[name] = (sizes.get(name, 0), h.hexdigest())
            name, h = m.group(1), hashlib.sha256()
            continue
        if name is None or not line.startswith(("\t", " ")):
            continue
        insn = re.sub(r"\s+", " ", line.split("//")[0]).strip()
        if insn:
            h.update(insn.encode() + b"\n")
    if name is not None:
        out[name] = (sizes.get(name, 0), h.hexdigest())
    return out


def digest(path):
    """[(name, size, sha256, {meta})] of every kernel in the file, sorted."""
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(path, tmp):
            meta, fns = kernel_meta(co), functions(co)
            for name, m in meta.items():
                size, sha = fns.get(name, (0, "-"))
                rows.append((name, size, sha, m))
    return sorted(rows, key=lambda r: (r[0], r[2]))


def demangled(names):
    tool = shutil.which("llvm-cxxfilt", path=llvm_bin()) or shutil.which("c++filt")
    names = list(names)
    if not names or tool is None:          # (no demangler: the mangled names)
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names).encode(), check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
    return dict(zip(names, out))


def fmt(row, pretty):
    name, size, sha, m = row
    figures = " ".join(f"{m.get(k, -1):6d}" for k in META)
    return f"{size:8d} {figures}  {sha}  {pretty[name]}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("files", nargs="+", help="built .o / .so files; with two, their differences are printed")
    args = ap.parse_args()
    tables = [digest(f) for f in args.files]
    pretty = demangled({r[0] for t in tables for r in t})
    head = f"{'bytes':>8s} {'vgpr':>6s} {'agpr':>6s} {'sgpr':>6s} {'scratch':>6s} {'lds':>6s}  sha256 of the disassembly" + " " * 39 + "kernel"
    if len(args.files) != 2:
        for f, t in zip(args.files, tables):
            print(f"# {f}: {len(t)} kernels")
            print(head)
            for r in t:
                print(fmt(r, pretty))
        return 0
    by = [{}, {}]
    for side, t in zip(by, tables):
        for r in t:
            side.setdefault(r[0], []).append(r)
    differ = 0
    for name in sorted(set(by[0]) | set(by[1])):
        a, b = by[0].get(name, []), by[1].get(name, [])
        if [r[1:] for r in a] == [r[1:] for r in b]:
            continue
        if not differ:
            print(head)
        differ += 1
        for tag, rows in (("<", a), (">", b)):
            for r in rows:
                print(tag, fmt(r, pretty))
            if not rows:
                print(tag, "(absent)", pretty[name])
    print(f"# {args.files[0]}: {len(tables[0])} kernels; {args.files[1]}: {len(tables[1])} kernels; {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
