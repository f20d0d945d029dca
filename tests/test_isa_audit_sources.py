"""Device-code audit of the sources' translation unit (csrc/sources.hip), on one compile of its gfx950 ISA, no GPU: its kernels
are the ones listed in tests/golden/device_kernels_sources.txt; every barrier -- the one inside the workgroup rank of the block
count and of the index kernel, the scan's -- has its LDS drain in front; and no kernel of the unit uses scratch memory: the
sinks, the face and the array tables travel in the kernel arguments and are indexed at compile-time positions."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_sources.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="sources.hip")


def test_the_sources_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name in ("14k_sources_emit", "12k_sink_count", "11k_sink_flag", "13k_sink_blocks", "11k_sink_scan", "12k_sink_index",
                 "13k_sink_gather"):
        assert sum(name in k for k in got) == 1, name


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    assert total >= 3  # the rank's barrier in the block count and in the index kernel, the scan's
    assert not bad, bad


def test_no_kernel_of_the_unit_uses_scratch():
    import isa_audit
    asm = _asm()
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, re.M)
    assert len(sizes) == len(isa_audit.kernel_names(asm)) == 7
    assert all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"^\s*scratch_", asm, re.M)
