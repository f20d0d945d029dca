"""Device-code audit of the fluid-surface translation unit (csrc/surface.hip), on one compile of its gfx950 ISA, no GPU: its
kernels are the ones listed in tests/golden/device_kernels_surface.txt (the lists of the other units do not change with
them); every barrier has its LDS drain in front; and no kernel of the unit uses scratch memory -- the emit kernel indexes
its cube's corners by table entries, which it does in LDS and with selects, never in a register array."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_surface.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="surface.hip")


def test_the_surface_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name in ("15k_surface_count", "19k_surface_scan_sums", "20k_surface_scan_apply", "14k_surface_emit"):
        assert sum(name in k for k in got) == 1, name


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    # count: behind the staging, behind the wave sums; emit: behind the staging, inside the prefix; one in each scan kernel
    assert total >= 6
    assert not bad, bad


def test_no_kernel_of_the_unit_uses_scratch():
    import isa_audit
    asm = _asm()
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, re.M)
    assert len(sizes) == len(isa_audit.kernel_names(asm)) == 4
    assert all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"^\s*scratch_", asm, re.M)
