"""Device-code audit of the rigid bodies' translation unit (csrc/bodies.hip), on one compile of its gfx950 ISA, no GPU: its
kernels are the ones listed in tests/golden/device_kernels_bodies.txt (csrc/sdf.hip and csrc/sdf_rigid.hip keep their own
lists); every barrier -- the tree's in the pass and in the fold, and the ones inside the workgroup vote of the loop over the
bodies -- has its LDS drain in front; and no kernel of the unit uses scratch memory: the particle, the record's words and the
six sums stay in registers."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_bodies.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="bodies.hip")


def test_the_bodies_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name in ("13k_bodies_pass", "12k_body_query", "13k_bodies_fold"):
        assert sum(name in k for k in got) == 1, name


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    assert total >= 2  # the tree's barrier in the pass and in the fold (the workgroup vote brings its own)
    assert not bad, bad


def test_no_kernel_of_the_unit_uses_scratch():
    import isa_audit
    asm = _asm()
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, re.M)
    assert len(sizes) == len(isa_audit.kernel_names(asm)) == 3
    assert all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"^\s*scratch_", asm, re.M)
