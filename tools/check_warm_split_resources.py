"""Registers, scratch and occupancy of the two-kernel warm-up (warm_score5_kernel, warm_select5_kernel in pda_amd/csrc/pda_score_topk_v4.hip),
read from hipcc -Rpass-analysis=kernel-resource-usage and held against the figures of profiles/warm_split.txt section 4.

The score kernel's loop fits its 256 registers only through a few scheduling fences and an empty asm statement per half-tile; another
compiler may decide otherwise, and nothing else would show it.  Run after a change to these kernels or to the compiler (no GPU needed; the
build must have run once, for the generated header):

    python tools/check_warm_split_resources.py            # compiles the device code of the file again (minutes)
    python tools/check_warm_split_resources.py LOG        # or reads the remarks of an earlier compilation

Exit status 1 when a kernel needs more than its limit."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pda_amd", "csrc", "pda_score_topk_v4.hip")
# kernel (substring of the mangled name) -> limits: VGPRs at most, scratch bytes per lane at most, occupancy (waves per SIMD) at least
LIMITS = {
    "warm_select5_kernel": (64, 0, 8),              # written for eight waves per SIMD
    "warm_score5_kernelILi64ELb0": (256, 0, 2),
    "warm_score5_kernelILi64ELb1": (256, 0, 2),
    "warm_score5_kernelILi128ELb0": (256, 124, 2),  # (scratch touched once per 32-user unit, none in the half-tile loop: an open item)
    "warm_score5_kernelILi128ELb1": (256, 224, 2),
}


def remarks():
    if len(sys.argv) > 1:
        return open(sys.argv[1]).read()
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", os.devnull]
    return subprocess.run(cmd, cwd=os.path.dirname(SRC), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout


def main():
    found, name = {}, None
    for line in remarks().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark: \s*(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            found.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    bad = 0
    for key, (vgprs, scratch, occ) in LIMITS.items():
        hits = [(n, r) for n, r in found.items() if key in n]
        if len(hits) != 1:
            print("%-32s not found in the remarks" % key)
            bad += 1
            continue
        r = hits[0][1]
        ok = r["VGPRs"] <= vgprs and r["ScratchSize"] <= scratch and r["Occupancy"] >= occ
        print("%-32s VGPRs %3d (<= %3d)  scratch %3d (<= %3d)  occupancy %d (>= %d)  %s" %
              (key, r["VGPRs"], vgprs, r["ScratchSize"], scratch, r["Occupancy"], occ, "ok" if ok else "OVER ITS LIMIT"))
        bad += 0 if ok else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
