"""Device-code audit of the contact stage's translation unit (csrc/contact.hip), on one compile of its gfx950 ISA, no GPU: its
kernels are the ones listed in tests/golden/device_kernels_contact.txt (csrc/bodies.hip keeps its own list); every barrier --
the trees' in the detection and in the fold, the scan's, the emit's, and the ones inside the workgroup votes and counts -- has
its LDS drain in front; and no kernel of the unit uses scratch memory: the point, the records' words and the nine sums stay
in registers."""
import functools
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels_contact.txt")


@functools.lru_cache(maxsize=None)
def _asm():
    import isa_audit
    return isa_audit.device_asm(source="contact.hip")


def test_the_contact_kernels_are_the_listed_ones():
    import isa_audit
    got = isa_audit.kernel_names(_asm())
    want = open(GOLDEN).read().split()
    assert got == want, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name in ("15k_contact_count", "14k_contact_scan", "14k_contact_emit", "16k_contact_detect", "14k_contact_fold", "15k_contact_solve"):
        assert sum(name in k for k in got) == 1, name


def test_every_barrier_has_its_lds_drain():
    import isa_audit
    bad, total = isa_audit.unprotected_barriers(_asm())
    assert total >= 4  # the tree's barrier in the detection and in the fold, the scan's, the emit's
    assert not bad, bad


def test_no_kernel_of_the_unit_uses_scratch():
    import isa_audit
    asm = _asm()
    sizes = re.findall(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, re.M)
    assert len(sizes) == len(isa_audit.kernel_names(asm)) == 6
    assert all(int(s) == 0 for s in sizes), sizes
    assert not re.search(r"^\s*scratch_", asm, re.M)
