#!/usr/bin/env python3
"""Is the device code of two builds of dslsph.hip the same, kernel by kernel?  (No GPU needed.)

A change to the host layer -- which instantiation a launch site picks, in which order the instantiations are named --
must leave every kernel as it was.  Both inputs are the gfx950 device assembly of the library's own flags:

  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -std=c++17 -S --cuda-device-only \\
        -o X.s dieselfluid_amd/csrc/dslsph.hip
  python tools/compare_device_asm.py parent.s branch.s      # exit code 1 on any difference

Each file is split at the `_ZN3dsl...:` labels up to the function's `.Lfunc_end`; `BB<digits>_` becomes `BB_` (the digits
are the function's emission index, which moves with the order of instantiation, in labels and in comments alike, and
with their number the padding in front of a label's comment); the bodies are compared per symbol.  A differing body means an instantiation or its arguments changed."""
import re
import sys

from isa_audit import demangle, kernel_names


def bodies(asm: str):
    out = {}
    for m in re.finditer(r"^(_ZN3dsl\w+):", asm, re.M):
        end = asm.find(".Lfunc_end", m.end())
        out[m.group(1)] = re.sub(r"[ \t]+;", " ;", re.sub(r"BB\d+_", "BB_", asm[m.end():end]))
    return out


def main():
    a, b = (open(p).read() for p in sys.argv[1:3])
    ba, bb = bodies(a), bodies(b)
    only_a, only_b = sorted(set(ba) - set(bb)), sorted(set(bb) - set(ba))
    differ = sorted(k for k in set(ba) & set(bb) if ba[k] != bb[k])
    dm = demangle(only_a + only_b + differ)
    for what, names in (("only in " + sys.argv[1], only_a), ("only in " + sys.argv[2], only_b), ("body differs", differ)):
        for k in names:
            print(f"{what}: {dm[k]}")
    same_kernels = kernel_names(a) == kernel_names(b)
    print(f"{len(ba)} / {len(bb)} symbols, {len(kernel_names(a))} / {len(kernel_names(b))} kernels, {len(differ)} bodies differ")
    return 1 if only_a or only_b or differ or not same_kernels else 0


if __name__ == "__main__":
    sys.exit(main())
