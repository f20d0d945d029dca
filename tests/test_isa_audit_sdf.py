"""Device-code audit of the implicit-collider translation unit (csrc/sdf.hip), on one compile of its gfx950 ISA, no GPU: its
kernels are the ones listed in tests/golden/device_kernels_sdf.txt (the lists of the other units do not change with it);
every barrier has its LDS drain in front; and no kernel of the unit uses scratch memory -- k_collide_volume holds its eight
corners in registers, k_sdf_sweep its three edges."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_sdf.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="sdf.hip")


def test_the_sdf_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name, count in (("10k_sdf_prep", 1), ("17k_sdf_brick_count", 1), ("16k_sdf_brick_fill", 1), ("14k_sdf_distance", 1),
                        ("11k_sdf_sweep", 1), ("10k_sdf_sign", 1), ("16k_collide_volume", 2)):
        assert sum(name in k for k in got) == count, name


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    assert total >= 2  # k_sdf_distance: behind the staging of a chunk, and behind its sweep (the next chunk overwrites it)
    assert not bad, bad


def test_no_kernel_of_the_unit_uses_scratch():
    import isa_audit
    asm = _asm()
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, re.M)
    assert len(sizes) == len(isa_audit.kernel_names(asm)) == 8
    assert all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"^\s*scratch_", asm, re.M)
