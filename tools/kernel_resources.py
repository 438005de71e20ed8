#!/usr/bin/env python3
"""Compares the kernels of two builds of the engine library by the resource
figures in their gfx950 code objects' metadata (VGPRs, SGPRs, scratch bytes
per lane, VGPR and SGPR spills, LDS bytes): the acceptance check that a
change left every existing kernel as it was.

  python tools/kernel_resources.py PARENT.so THIS.so

Prints one JSON object: the kernel counts, the kernels whose figures differ
(parent, this) and the kernels only THIS has.
"""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
        "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


def kernels(lib):
    """{kernel: KEYS' values} over every code object in lib's fat binary."""
    with tempfile.TemporaryDirectory() as d:
        return _kernels(lib, d)


def _kernels(lib, d):
    fat = os.path.join(d, "fat.bin")
    subprocess.check_call(["objcopy", "-O", "binary",
                           "--only-section=.hip_fatbin", lib, fat])
    data = open(fat, "rb").read()
    out, pos, n = {}, 0, 0
    while True:
        i = data.find(b"\x7fELF\x02\x01\x01\x40", pos)  # ELF64, AMDGPU HSA
        if i < 0:
            return out
        shoff = struct.unpack_from("<Q", data, i + 0x28)[0]
        shentsize, shnum = struct.unpack_from("<HH", data, i + 0x3A)
        end = i + shoff + shentsize * shnum
        p = os.path.join(d, "co%d.elf" % n)
        with open(p, "wb") as f:
            f.write(data[i:end])
        txt = subprocess.run([READELF, "--notes", p], capture_output=True,
                             text=True).stdout
        for blk in txt.split("- .agpr_count")[1:]:
            def g(k):
                m = re.search(r"\.%s:\s+(\S+)" % k, blk)
                return m.group(1) if m else None
            out[g("name")] = tuple(int(g(k)) if g(k) else -1 for k in KEYS)
        n += 1
        pos = end


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(json.dumps(dict(
        keys=KEYS, parent_kernels=len(a), this_kernels=len(b),
        differing={k: (a[k], b.get(k)) for k in a if a[k] != b.get(k)},
        new={k: b[k] for k in b if k not in a}), indent=1))


if __name__ == "__main__":
    main()
